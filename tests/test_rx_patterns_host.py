"""The burst detector's references and designed patterns on the CPU
(tests/rx_patterns.py; the GPU runs are tests/test_gpu_rx_shapes.py).

first_run is pinned to the reference's literal loop, scan_model (the three-level
search as k_bf_flags / k_bf_scan run it) to first_run, and a census keeps every
branch of the search hit by a designed pattern, each pattern on the branch it is
named after.  smooth_ref's centring of even windows is pinned to np.convolve's."""
import numpy as np
import pytest

import rx_patterns as RP

DESIGNED = RP.designed()
EPS = np.finfo(np.float64).eps
SMOOTH_WINS = (1, 2, 37, 999, 1000, 1024)
SMOOTH_NS = ("win", 1024, 1025, 4096, 4097)


def smooth_cases():
    return [(w, w if n == "win" else n) for w in SMOOTH_WINS for n in SMOOTH_NS if n == "win" or n >= w]


def test_flags_to_signal_is_exact():
    f = RP.random_flags(np.random.default_rng(1), 5000, 10)
    for dt in (np.complex64, np.complex128):
        x = RP.flags_to_signal(f, dt)
        assert x.dtype == dt and np.array_equal(np.abs(x) ** 2 > 0.3, f)
        # the DC case of the GPU test: adding and removing 0.25 + 0.5j is exact in both dtypes
        dc = dt(0.25 + 0.5j)
        assert np.array_equal((x + dc) - dc, x)


@pytest.mark.parametrize("p", [p for p in DESIGNED if p.n <= 8192], ids=repr)
def test_first_run_is_the_literal_loop_designed(p):
    assert RP.first_run(p.flags, p.pre) == RP.literal_first_run(p.flags, p.pre)


def test_first_run_is_the_literal_loop_random():
    rng = np.random.default_rng(20261019)
    for k in range(200):
        n = int(rng.choice([1, 5, 300, 1023, 1024, 1025, 3000]))
        pre = int(rng.choice([0, 1, 2, 3, 10, 64, 65, 700]))
        f = RP.random_flags(rng, n, pre // 2)
        assert len(f) == n
        assert RP.first_run(f, pre) == RP.literal_first_run(f, pre), (k, n, pre)


@pytest.mark.parametrize("p", DESIGNED, ids=repr)
def test_scan_model_designed(p):
    got, taken = RP.scan_model(p.flags, p.pre)
    assert got == RP.first_run(p.flags, p.pre)
    assert taken <= set(RP.BRANCHES)
    if p.branch is not None:
        assert p.branch in taken, (p.name, sorted(taken))


def test_scan_model_random():
    rng = np.random.default_rng(20261020)
    ns = (1, 5, 1023, 1024, 1025, 3000, 4097, 8192)
    pres = (0, 1, 2, 3, 10, 64, 65, 700, 2049, 5000)
    seen = set()
    for k in range(500):
        n, pre = ns[k % len(ns)], pres[(k // len(ns) + k) % len(pres)]
        f = RP.random_flags(rng, n, pre // 2)
        got, taken = RP.scan_model(f, pre)
        assert got == RP.first_run(f, pre), (k, n, pre)
        seen |= taken
    for pre in (64, 2049, 300000):
        f = RP.random_flags(rng, RP.BIG_N, pre // 2)
        f[:400 * RP.TILE:pre // 2] = False          # no qualifying run in the first pass
        got, taken = RP.scan_model(f, pre)
        assert got == RP.first_run(f, pre), pre
        assert "second_chunk" in taken
        seen |= taken
    print("branches of the random patterns:", sorted(seen))


def test_census_every_branch_is_hit():
    union = set()
    for p in DESIGNED:
        union |= RP.scan_model(p.flags, p.pre)[1]
    print("branches of the designed patterns:", sorted(union))
    assert union == set(RP.BRANCHES)
    # the named paths of the issue, each by a pattern built for it
    for name in ("cross_tile_run", "tile_local_start", "tile_without_zero", "second_chunk", "carry_used",
                 "tail_run", "limit_rejects"):
        assert any(p.branch == name for p in DESIGNED) or name == "second_chunk", name
    assert all("second_chunk" in RP.scan_model(p.flags, p.pre)[1] for p in DESIGNED if p.n == RP.BIG_N)
    # both sides of every exact-length edge give different answers
    by = {p.name: RP.first_run(p.flags, p.pre) for p in DESIGNED}
    for name, ans in by.items():
        if "_short-" in name:
            assert by[name.replace("_short-", "-")] != ans, name


@pytest.mark.parametrize("win,n", smooth_cases())
def test_smooth_ref_is_np_convolve(win, n):
    """The long double cumulative-sum form against numpy's own 'same' convolution, within the
    rounding of numpy's win-term dot product: win * eps * max(p)."""
    rng = np.random.default_rng(win * 10000 + n)
    for dt in (np.complex64, np.complex128):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dt)
        p = np.abs(x - np.mean(x)) ** 2
        assert p.dtype == (np.float32 if dt == np.complex64 else np.float64)
        ref = RP.smooth_ref(p, win)
        conv = np.convolve(p.astype(np.float64), np.ones(win) / win, "same")
        assert ref.shape == conv.shape == (n,)
        assert np.max(np.abs(ref - conv)) <= win * EPS * np.max(p)
