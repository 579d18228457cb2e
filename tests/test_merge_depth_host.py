"""Merge depths on the CPU: the oracle's siso_depths / decode_depths, the merge
argument itself, and the classes of every fixture the GPU tests rely on
(tests/merge_fixtures.py, tests/test_gpu_merge_depth.py).

The state vectors are not exported by the oracle, so the merge argument is
checked on an independent restatement: the numpy f32 pair-maxima recursion of
tests/frame_model.py (serial_pass), fed with the branch metrics of the same
SISO row.  Its depths must equal the oracle's, and past a depth every vector of
the second pass must equal the first pass's."""
import numpy as np
import pytest

import merge_fixtures as F
import frame_model as FM
from oracle import oracle as O

TAB, _ = O.trellis()


def pair_maxima(LcA, LcB, LcW, LcY, LaA, LaB):
    """Max-log branch metrics of a SISO row as the pair maxima pm [N][8] the frame
    model takes: index (c << 2) | (w << 1) | y holds the larger of the two parallel
    branches of input class c = A ^ B with parity bits (w, y); each branch is the
    reference's f64 sum in its order (dvb_rcs2_turbo.py:127-160), stored f32."""
    inA = np.asarray(LcA, np.float64) + LaA
    inB = np.asarray(LcB, np.float64) + LaB
    W, Y = np.asarray(LcW, np.float64), np.asarray(LcY, np.float64)
    pm = np.zeros((len(inA), 8), np.float32)
    sg = lambda b: 0.5 if b == 0 else -0.5   # noqa: E731
    for c in range(2):
        for w in range(2):
            for y in range(2):
                br = []
                for a in range(2):
                    b = a ^ c
                    m = np.zeros(len(inA))
                    m = m + inA * sg(a)
                    m = m + inB * sg(b)
                    m = m + W * sg(w)
                    m = m + Y * sg(y)
                    br.append(m.astype(np.float32))
                pm[:, (c << 2) | (w << 1) | y] = np.maximum(br[0], br[1])
    return pm


def model_vectors(pm, beta):
    """([N + 1][16] pass 1, pass 2) of the model, in step order (row u: the vector
    after u steps from the pass's start; backward passes start at the top)."""
    s1, e1 = FM.serial_pass(pm, np.zeros(16, np.float32), beta)
    s2, e2 = FM.serial_pass(pm, e1, beta)
    return np.vstack([s1, e1[None]]), np.vstack([s2, e2[None]])


def model_depth(v1, v2):
    eq = np.all(v1 == v2, axis=1)
    return int(np.argmax(eq)) if eq.any() else -1


def _check_row(row, want=None):
    depths = O.siso_depths(*row, TAB, 0.7)
    if want is not None:
        assert depths == want
    pm = pair_maxima(*row)
    for beta, d in zip((False, True), depths):
        v1, v2 = model_vectors(pm, beta)
        assert model_depth(v1, v2) == d          # the oracle's depth, from an independent restatement
        if d >= 0:
            np.testing.assert_array_equal(v2[d:], v1[d:])   # merged once, merged for good
        else:
            assert not np.all(v1 == v2, axis=1).any()
    return depths


@pytest.mark.parametrize("n", [5, 48, 100, 212])
def test_merge_argument_random_rows(n):
    rng = np.random.default_rng(n)
    for scale in (0.5, 3.0):
        Lc = [(rng.standard_normal(n) * scale).astype(np.float32) for _ in range(4)]
        La = [rng.standard_normal(n) * 2 * scale for _ in range(2)]
        f2, b2 = _check_row((*Lc, *La))
        assert -1 <= f2 <= n and -1 <= b2 <= n


def test_depths_do_not_depend_on_sf_or_dtype_and_nan_never_merges():
    n = 100
    rng = np.random.default_rng(1)
    Lc = [(rng.standard_normal(n) * 2).astype(np.float32) for _ in range(4)]
    La = [rng.standard_normal(n) * 4 for _ in range(2)]
    d = O.siso_depths(*Lc, *La, TAB, 0.7)
    assert d == O.siso_depths(*Lc, *La, TAB, 1.0)
    assert d == O.siso_depths(*(x.astype(np.float64) for x in Lc), *La, TAB, 0.7)
    # a NaN a-priori value poisons every later vector of both passes: C == is never true
    La[0][:] = np.nan
    assert O.siso_depths(*Lc, *La, TAB, 0.7, 1) == (-1, -1)
    # zero input: both passes stay at zero, merged at step 0
    z32, z64 = np.zeros(n, np.float32), np.zeros(n)
    assert O.siso_depths(z32, z32, z32, z32, z64, z64, TAB, 0.7) == (0, 0)


def test_depth_entry_points_leave_the_outputs_alone():
    """siso() / decode() before and after a depths call: the same arrays."""
    from modulations_amd import dvb_rcs2_turbo as M
    from modulations_amd import tables as T
    c = M.DVBRCS2_Turbo(48, "1/2")
    llr = F.decode_llr(c, "never", 0)
    args = (llr, 48, c.punct["period"], T.puncture_matrix(c.punct), 3, c.perm, c.inv_perm, TAB)
    b0, l0 = O.decode(*args, want_lfinal=True)
    d = O.decode_depths(*args)
    assert d.shape == (3, 2, 2) and d.dtype == np.int32
    b1, l1 = O.decode(*args, want_lfinal=True)
    np.testing.assert_array_equal(b0, b1)
    np.testing.assert_array_equal(l0, l1)
    # iteration 1 of decoder 1 is the SISO on the de-punctured planes with zero a-priori
    pl = O.depuncture(llr, 48, c.punct["period"], T.puncture_matrix(c.punct))
    z = np.zeros(48)
    assert tuple(d[0, 0]) == O.siso_depths(pl[0], pl[1], pl[2], pl[3], z, z, TAB, 0.7)
    with pytest.raises(IndexError):
        O.decode_depths(llr[:-1], *args[1:])


def test_exact_reference_keeps_its_route_and_reports_no_depths():
    """algo 2 is the exact f64 log-MAP in siso() and in decode() alike: decode(algo=2)
    equals the decode assembled from siso(algo=2) calls (dvb_rcs2_turbo.py:464-537), and
    differs from the build's f32 log-MAP (algo 1).  It keeps no pass-1 copy, so the
    depth entry points refuse it instead of answering for another algorithm."""
    from modulations_amd import dvb_rcs2_turbo as M
    from modulations_amd import tables as T
    n, iters = 48, 3
    c = M.DVBRCS2_Turbo(n, "1/2")
    pm = T.puncture_matrix(c.punct)
    llr = (np.random.default_rng(7).standard_normal(4 * n) * 3).astype(np.float32)
    args = (llr, n, c.punct["period"], pm, iters, c.perm, c.inv_perm, TAB)
    A, B, W1, Y1, W2, Y2 = O.depuncture(llr, n, c.punct["period"], pm)
    LaA, LaB = np.zeros(n), np.zeros(n)
    for it in range(iters):
        sf = 0.7 if it < iters - 1 else 1.0
        Le1A, Le1B = O.siso(A, B, W1, Y1, LaA, LaB, TAB, sf, 2)
        Le2A, Le2B = O.siso(A[c.perm], B[c.perm], W2, Y2, Le1A[c.perm], Le1B[c.perm], TAB, sf, 2)
        LaA, LaB = Le2A[c.inv_perm], Le2B[c.inv_perm]
    want = np.stack([(A.astype(np.float64) + LaA) + Le1A, (B.astype(np.float64) + LaB) + Le1B], axis=1).ravel()
    bits, lf = O.decode(*args, algo=2, want_lfinal=True)
    np.testing.assert_array_equal(lf, want)
    np.testing.assert_array_equal(bits, (want < 0).astype(np.int32))
    assert not np.array_equal(lf, O.decode(*args, algo=1, want_lfinal=True)[1])
    with pytest.raises(ValueError):
        O.decode_depths(*args, algo=2)
    with pytest.raises(ValueError):
        O.siso_depths(A, B, W1, Y1, LaA, LaB, TAB, 0.7, 2)


@pytest.mark.parametrize("n", sorted(F.SISO_SEEDS))
def test_siso_fixture_classes_and_merge_argument(n):
    """Every SISO fixture row: finite small integers, in the class its GPU test
    relies on, and merged for good past its depth (model and oracle agree)."""
    Lc, La, meta = F.siso_batch(n)
    assert len(meta) <= 8
    seen = {"f2": set(), "b2": set()}
    for r, (fam, seed, which, cls) in enumerate(meta):
        row = tuple(x[r] for x in Lc + La)
        for x in row:
            assert np.all(np.isfinite(x)) and np.all(x == np.rint(x)) and np.abs(x).max() <= F.STRETCH
        f2, b2 = _check_row(row)
        print(f"N={n} {fam} seed {seed}: f2 {f2} b2 {b2}")
        if which in ("f2", "both"):
            assert F.depth_class(n, f2) == cls, (fam, f2)
            seen["f2"].add(cls)
        if which in ("b2", "both"):
            assert F.depth_class(n, b2) == cls, (fam, b2)
            seen["b2"].add(cls)
        if which is None:   # plain rows merge early, like noisy traffic
            assert 0 <= f2 <= 128 and 0 <= b2 <= 128
    want = {"a", "b", "c", "d"} if n >= F.FAR else {"a", "b", "d"}
    assert seen["f2"] == want and seen["b2"] == want


def test_depth_classes_follow_the_kernels_grids():
    # N % 8 == 0: both rings compare every 16 steps down to 240 (the top 256 steps)
    assert F.b2_checks(752, F.CK8, F.RSTEP8) == list(range(0, 256, 16))
    assert F.b2_checks(752, F.WIN, F.rstep_of(F.WIN)) == list(range(0, 256, 16))
    assert F.ring_reach(752) == (240, 240)
    # ragged: the short top window shifts the grid (790 = 98 * 8 + 6 = 197 * 4 + 2)
    assert F.b2_checks(790, F.CK8, F.RSTEP8)[:3] == [0, 14, 30]
    assert F.b2_checks(790, F.WIN, 4)[:3] == [0, 14, 30]
    # shorter than the ring: the last kept window start that exists
    assert F.ring_reach(212) == (204, 208)
    assert [F.depth_class(752, d) for d in (-1, 233, 240, 241, 304, 305, 700, 752)] == \
        ["d", "a", None, "b", "b", None, "c", "c"]
    assert F.depth_class(752, 224) is None and F.depth_class(752, 236) is None   # on a grid
    assert (F.fr_seg_len(752, 4), F.fr_seg_len(752, 8), F.fr_seg_len(220, 4), F.fr_seg_len(48, 4)) == (188, 96, 56, 48)


@pytest.mark.parametrize("key", sorted(F.DECODE_SEEDS))
def test_decode_fixture_classes(key):
    """Every decode fixture: each never-merging vector keeps all its SISO calls --
    all 8 iterations, both decoders, both directions -- in class (c) or (d); the
    class (b) vector has decoder 1's B2 just past the ring in iteration 1 and in a
    later one; L_final stays far inside the +-300 clip."""
    from modulations_amd import dvb_rcs2_turbo as M
    from modulations_amd import tables as T
    n, rate = key
    c = M.DVBRCS2_Turbo(n, rate)
    args = (n, c.punct["period"], T.puncture_matrix(c.punct), 8, c.perm, c.inv_perm, TAB)
    s = F.DECODE_SEEDS[key]
    for seed in s["never"]:
        llr = F.decode_llr(c, "never", seed)
        assert np.all(np.isfinite(llr)) and np.all(llr == np.rint(llr))
        d = O.decode_depths(llr, *args)
        print(f"N={n} r={rate} never seed {seed}: {d.reshape(8, 4).tolist()}")
        assert all(F.depth_class(n, int(x)) in ("c", "d") for x in d.ravel())
        _, lf = O.decode(llr, *args, want_lfinal=True)
        assert np.abs(lf).max() < 150.0
    d = O.decode_depths(F.decode_llr(c, *s["b"]), *args)
    print(f"N={n} r={rate} {s['b']}: {d.reshape(8, 4).tolist()}")
    assert F.depth_class(n, int(d[0, 0, 1])) == "b"
    assert any(F.depth_class(n, int(d[it, 0, 1])) == "b" for it in range(1, 8))
    d = O.decode_depths(F.decode_llr(c, "plain", 0), *args)
    assert d.min() >= 0   # plain vectors always merge


@pytest.mark.parametrize("n,P", [(212, 4), (212, 8), (752, 4), (752, 8)])
@pytest.mark.parametrize("beta", [False, True])
def test_frame_model_on_the_finite_never_merging_row(n, P, beta):
    """The frame decoder's segment rounds (tests/frame_model.py) on the finite
    row that never merges: no segment merges in any round, every one hands its end
    vector on, and the stored vectors are the serial two passes.  Each round
    settles at least one more segment of the chain: the first pass's chain is
    right after nseg - 1 rounds (segment 0 starts from zero), the second pass's
    after nseg more, so 2 nseg - 1 rounds is the most any input can need."""
    row = F.siso_rows(n, "never", F.SISO_SEEDS[n][-2 if n != 212 else 4][1])
    assert O.siso_depths(*row, TAB, 0.7) == (-1, -1)
    pm = pair_maxima(*row)
    st, stats = FM.frame_recursion(pm, beta, P, F.FR_LMIN)
    np.testing.assert_array_equal(st, FM.reference_two_pass(pm, beta))
    Ls = F.fr_seg_len(n, P)
    nseg = -(-n // Ls)
    print(f"N={n} P={P} beta={beta}: {stats['rounds']} rounds, {nseg} segments of {Ls}")
    assert stats["rounds"] <= 2 * nseg - 1
