"""The case tables of tests/modem_edges.py, checked on the CPU: every numpy restatement equals
the C oracle on every case, the integer FIR sums are exact, the tables reach every kernel
instantiation and branch they are there for, and every family tells its operation from a near
miss -- a deliberately wrong numpy variant must differ from the reference on at least one case
of each family that claims to cover it.  Nothing here is built for or run on a GPU."""
import numpy as np
import pytest

import modem_edges as E
from oracle import oracle as O
from test_modem_host import psk8_boundary_ok

C64, C128 = E.C64, E.C128


# ---------------------------------------------------------------- FIR -------------------------
@pytest.mark.parametrize("family", E.FIR_FAMILIES)
def test_fir_reference_equals_oracle_and_stays_exact(family):
    for c in E.fir_cases(family):
        x, h = E.fir_inputs(c)
        assert x.dtype == c.dtype and len(x) == c.n_x and len(h) == c.n_taps
        assert np.array_equal(x, np.round(x)) and np.array_equal(h, np.round(h))
        # every partial sum is bounded by sum|h| max|x|: an exact double
        assert np.abs(h).sum() * max(np.abs(x.real).max(), np.abs(x.imag).max()) < 2.0 ** 53
        ref = E.fir_case_ref(c)
        assert E.same_bits(ref, O.modem_fir(x, h, c.up, c.down, c.offset, c.n_out)), c
        assert not ref[E.n_valid(c):].any()


def test_fir_tables_reach_every_kernel_and_edge():
    by = {f: {E.fir_kernel(c) for c in E.fir_cases(f)} for f in E.FIR_FAMILIES}
    ts = ("float", "double")
    assert by["up"] == {f"k_fir_up<{t},{u}>" for t in ts for u in (2, 4, 8, 16)}
    assert by["dec"] == {f"k_fir_dec<{t},{d}>" for t in ts for d in (1, 2, 4, 8)}
    assert by["staged"] == {f"k_fir<{t},true>" for t in ts}
    assert by["unstaged"] == {f"k_fir<{t},{s}>" for t in ts for s in ("true", "false")}
    assert by["stride"] == {"k_fir_up<float,2>", "k_fir_dec<float,1>"}
    assert all(E.fir_second_trip(c) for c in E.fir_cases("stride"))
    assert not any(E.fir_second_trip(c) for f in E.FIR_FAMILIES[:4] for c in E.fir_cases(f))
    # the staging threshold: down 15 with 13 and 14 taps staged, 15 taps not
    thr = {(c.n_taps, E.fir_kernel(c)[-6:]) for c in E.fir_cases("unstaged") if c.down == 15}
    assert thr == {(13, ",true>"), (14, ",true>"), (15, "false>")}
    assert {c.n_out for c in E.fir_cases("unstaged")} == {3 * E.BLOCK + 5}
    # per_thread = 4 (down 1) and 1, output counts around a block's, several blocks
    for up, down, opb in ((3, 2, 256), (5, 3, 256), (2, 3, 256), (3, 1, 1024), (7, 1, 1024)):
        got = {c.n_out for c in E.fir_cases("staged") if (c.up, c.down) == (up, down)}
        assert got == {opb - 1, opb, opb + 1, 3 * opb + 5}
    for f in ("up", "dec"):
        cs = E.fir_cases(f)
        for k in {E.fir_kernel(c) for c in cs}:
            mine = [c for c in cs if E.fir_kernel(c) == k]
            assert any(c.n_out > E.n_valid(c) for c in mine), k            # runs past the end
            assert any(c.n_out == E.n_valid(c) for c in mine), k           # ends with it
            assert any(c.offset > c.n_taps - 1 for c in mine), k
            assert any(c.n_x < c.n_taps for c in mine) and any(c.n_x == 1 for c in mine), k
            assert {1, 256} <= {c.n_taps for c in mine}, k
    assert 300 <= sum(len(E.fir_cases(f)) for f in E.FIR_FAMILIES) <= 700
    assert {E.fir_kernel(c) for c in E.FIR_REAL} >= {"k_fir_up<float,4>", "k_fir_up<double,2>", "k_fir_dec<double,2>",
                                                     "k_fir_dec<float,1>", "k_fir<float,true>", "k_fir<double,false>"}


FIR_MISSES = {"offset+1": E.FIR_FAMILIES, "phase": ("up", "staged", "stride"), "drop_last_tap": E.FIR_FAMILIES,
              "past_end": ("up", "dec", "staged", "unstaged", "stride")}


@pytest.mark.parametrize("variant", sorted(FIR_MISSES))
def test_fir_cases_catch_near_misses(variant):
    for family in FIR_MISSES[variant]:
        assert any(not E.same_bits(E.fir_case_ref(c), E.fir_case_ref(c, variant)) for c in E.fir_cases(family)), family


def test_fir_near_misses_are_near():
    """Each variant agrees with the reference somewhere: it is a subtle error, not a different operation."""
    cs = [c for f in E.FIR_FAMILIES[:4] for c in E.fir_cases(f)]
    for variant in FIR_MISSES:
        same = sum(np.sum(E.fir_case_ref(c) == E.fir_case_ref(c, variant)) for c in cs[::7])
        assert same > 0, variant


# ---------------------------------------------------------------- mapper ----------------------
def test_map_reference_equals_oracle():
    seen = set()
    for c in E.map_cases() + E.MAP_LARGE:
        bits, table = E.map_inputs(c)
        assert len(set(table.tolist())) == 1 << c.bps and table.dtype == c.dtype
        ref = E.map_ref(bits, c.bps, table)
        assert E.same_bits(ref, O.modem_map(bits, c.bps, table)), c
        seen.add((c.bps, c.dtype))
    assert seen == {(b, C64) for b in range(1, 9)} | {(b, C128) for b in range(1, 8)}
    assert all(c.n_bits > E.MAP_GRID * E.MAP_SPB * c.bps for c in E.MAP_LARGE)        # the s0 loop's second trip


@pytest.mark.parametrize("variant", ["lsb_first", "pad_ones"])
def test_map_cases_catch_near_misses(variant):
    for dt in (C64, C128):
        cs = [c for c in E.map_cases() if c.dtype == dt]
        assert any(not E.same_bits(E.map_ref(*_m(c)), E.map_ref(*_m(c), variant)) for c in cs)


def _m(c):
    bits, table = E.map_inputs(c)
    return bits, c.bps, table


# ---------------------------------------------------------------- hard demodulators -----------
def _oracle(c):
    return O.modem_demod(c.syms, c.kind, c.bps, labels=c.labels, scale=c.scale, cons=c.cons,
                         nan_raises=bool(c.nan_raises))


@pytest.mark.parametrize("family", E.DEMOD_FAMILIES)
def test_demod_reference_equals_oracle(family):
    for c in E.demod_cases(family):
        bits, nans = E.demod_ref(c)
        obits, onans = _oracle(c)
        assert nans == onans, c.name
        if family == "psk8_boundary":
            psk8_boundary_ok(c.syms, bits, obits)
        else:
            assert np.array_equal(bits, obits), c.name
    if family == "argmin":
        c = E.demod_large("qam256")
        assert np.array_equal(E.demod_ref(c)[0], _oracle(c)[0])
        c = E.demod_large("gt0")
        assert np.array_equal(E.demod_ref(c)[0], _oracle(c)[0])


def test_qam_axis_cases_sit_on_the_ties():
    for c in E.demod_cases("qam_axis"):
        if "NaN" in c.name:
            assert E.demod_ref(c)[1] == 2 + 2 + 2            # (nan, nan) twice, one axis only four times
            continue
        L = 1 << (c.bps // 2)
        for part in (c.syms.real, c.syms.imag):
            p = E.qam_axis_position(part, c.bps, c.scale)
            assert np.isinf(p).sum() == 2
            p = np.where(np.isinf(p), np.sign(p) * 1e300, p)
            ties, ints = set(p[np.mod(p, 1.0) == 0.5]), set(p[np.mod(p, 1.0) == 0.0]) - {np.inf, -np.inf}
            if c.scale == 2.0:                               # every one of them, exactly
                assert ties >= set(np.arange(-0.5, L, 1.0)) and ints >= set(np.arange(-1.0, L + 1))
            else:                                            # those that a float reaches
                assert len(ties) >= 1 and len(ints) >= 1
            assert np.isinf(part).sum() == 2 and (p > L + 2).sum() == 2 and (p < -3).sum() == 2


def test_argmin_ties_are_exact():
    for c in E.demod_cases("argmin"):
        if "ties" not in c.name:
            continue
        d = np.abs(c.syms.astype(C128)[:, None] - c.cons[None, :])
        n_min = (d == d.min(1, keepdims=True)).sum(1)
        assert 2 in n_min and (c.bps == 1 or 4 in n_min), c.name


DEMOD_MISSES = {"half_away": "qam_axis", "no_clip": "qam_axis", "last_min": "argmin"}


@pytest.mark.parametrize("variant", sorted(DEMOD_MISSES))
def test_demod_cases_catch_near_misses(variant):
    cs = E.demod_cases(DEMOD_MISSES[variant])
    for dt in (C64, C128):
        for bps in {c.bps for c in cs}:
            mine = [c for c in cs if c.syms.dtype == dt and c.bps == bps]
            assert any(not np.array_equal(E.demod_ref(c)[0], E.demod_ref(c, variant)[0]) for c in mine), (dt, bps)


# ---------------------------------------------------------------- IQ formats ------------------
@pytest.mark.parametrize("dt", [C64, C128])
def test_quant_reference_equals_oracle(dt):
    cases = E.quant_cases(dt)
    assert set(cases) == set(E.QUANT_NAMES) - ({"denormal"} if dt == C128 else set())
    for name, sig in cases.items():
        assert sig.dtype == dt
        assert np.array_equal(E.quant_ref(sig), O.modem_iq_quantize(sig)), name
    T, m = E._real(dt), E.QUANT_MARGIN[dt]
    for name in ("circle", "near_circle", "long"):           # many samples within the margin of the maximum
        q = np.abs(cases[name].astype(C128)) ** 2
        assert (q >= (1 - m) * q.max()).sum() >= 1000, name
    assert len(cases["long"]) > 2 * E.STRIDE
    st = cases["steps"]                                      # on, below and above every integer up to 120
    d = T(np.abs(st).max()) + T(1e-10)
    for part in (st.real, st.imag):
        v = E._quant_scaled(part, d, T)
        for s in (v, -v):                                    # four roundings: a float lands on most integers, not all
            assert sum((s == k).any() for k in range(1, 121)) >= 100
            for k in range(1, 121):
                assert ((np.trunc(s) == k - 1) & (s > k - 1e-3)).any() and ((np.trunc(s) == k) & (s < k + 1e-3)).any(), k
    assert np.abs(E.quant_ref(st)).max() == 120


@pytest.mark.parametrize("variant", ["round", "skip_max"])
def test_quant_cases_catch_near_misses(variant):
    for dt in (C64, C128):
        cases = E.quant_cases(dt)
        names = ("gauss", "steps") if variant == "round" else ("gauss", "steps", "long")
        for name in names:
            assert not np.array_equal(E.quant_ref(cases[name]), E.quant_ref(cases[name], variant)), (dt, name)


def test_dequant_reference_equals_oracle_and_catches_near_misses():
    cases = E.dequant_cases()
    assert len(cases["all pairs"]) == 2 * 65536 and len(set(map(tuple, cases["all pairs"].reshape(-1, 2)))) == 65536
    for name, raw in cases.items():
        ref = E.dequant_ref(raw)
        assert E.same_bits(ref, O.modem_iq_dequantize(raw)), name
        for mid in (127, 128):
            assert not np.array_equal(ref, E.dequant_ref(raw, mid)), (name, mid)
    assert sum(a % 16 == 0 and 8 * b % 16 == 0 for a, b in E.DEQUANT_OFFSETS) == 2
