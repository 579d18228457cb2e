"""The merge shortcuts on finite inputs that merge late, or never.

Every decoder skips the rest of a second recursion pass once it equals the first
(DESIGN.md §3), each kernel by its own shortcut: siso8 and siso<0, 4> stop per lane
at a checkpoint and test B2 against a ring of kept beta1 vectors that covers only
the top RING * 16 steps; the frame decoder re-runs segments until they merge and
hands end vectors down the chain; the low-latency decoder overwrites its stored
vectors until equal; the state-per-lane prototype stops a whole wave.  Noisy rows
merge within ~200 steps, and the NaN fixtures that never merge compare NaN with
NaN, so the deep ends of those paths -- B2 past the ring, a lane hundreds of steps
behind its wave-mates, a chain in which no segment merges, a pass 2 that rewrites
the whole store -- need the finite fixtures of tests/merge_fixtures.py.

Every comparison is against the C oracle by np.testing.assert_array_equal (bits,
L_final, extrinsics: no tolerances), and every test first asserts, from
oracle.siso_depths / decode_depths, that its rows are in the depth class it is
there for.  The classes (a) inside the ring's reach and off the grid, (b) just
past the ring, (c) far past (>= 700), (d) never, are computed from the kernels'
constants, restated with file and line in merge_fixtures.py (RING, rstep_of, the
8-step checkpoint, fr_seg_len) and checked on the CPU by
tests/test_merge_depth_host.py."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("trans_tables")]

import early_stop_ref as R  # noqa: E402
import merge_fixtures as F  # noqa: E402
from oracle import oracle as O  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402

TAB, _ = O.trellis()
_C48 = M.DVBRCS2_Turbo(48, "1/3")
TABLES = (_C48.next_state, _C48.out_W, _C48.out_Y, _C48.prev_state, _C48.prev_input)
SISO_N = [212, 752, 790, 848]          # 790: ragged windows; 848: Le2 in global memory at decode level
DECODE_SHAPES = [(752, "1/3"), (220, "1/2"), (848, "1/3")]   # 220 = 27 * 8 + 4: ragged checkpoints


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- SISO level ------------------------------------------------------------------------

def _assert_siso_classes(n, algo=0):
    """The batch holds every class for F2 and for B2 (max-log: exact small-integer
    arithmetic, the depths pinned on the CPU).  log-MAP's depths depend on the
    device's exp2 / log2 tables, so there only the rows that cannot merge are
    asserted: a stretch is a permutation for max* as well (the correction of a
    branch 64 behind is absorbed), classes (c) / (d)."""
    Lc, La, meta = F.siso_batch(n)
    seen = {"f2": set(), "b2": set()}
    for r, (fam, seed, which, cls) in enumerate(meta):
        f2, b2 = O.siso_depths(*(x[r] for x in Lc + La), TAB, 0.7, algo)
        for key, d in (("f2", f2), ("b2", b2)):
            if which in (key, "both"):
                if algo == 0:
                    assert F.depth_class(n, d) == cls, (n, fam, key, d)
                seen[key].add(F.depth_class(n, d))
    if algo == 0:
        want = {"a", "b", "c", "d"} if n >= F.FAR else {"a", "b", "d"}
        assert seen["f2"] == want and seen["b2"] == want
    else:
        assert seen["f2"] & {"c", "d"} and seen["b2"] & {"c", "d"}, seen


@functools.lru_cache(maxsize=None)
def _siso_ref(n, f64, sf, algo):
    Lc, La, _ = F.siso_batch(n, f64)
    ref = [O.siso(*(x[r] for x in Lc + La), TAB, sf, algo) for r in range(Lc[0].shape[0])]
    out = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    for x in out:
        x.setflags(write=False)
    return out


def _check_siso(n, f64, sf, algo=0):
    Lc, La, _ = F.siso_batch(n, f64)
    LeA, LeB = M.bcjr_max_log_map_batch(*Lc, *La, *TABLES, n, sf, algo="log-map" if algo else "max-log")
    rA, rB = _siso_ref(n, f64, sf, algo)
    np.testing.assert_array_equal(LeA, rA)
    np.testing.assert_array_equal(LeB, rB)


@pytest.mark.parametrize("n", SISO_N)
@pytest.mark.parametrize("kernel", ["frame-one", "frame-two", "row", "spl"])
def test_siso_every_depth_class(n, kernel, monkeypatch):
    """One batch of at most 8 rows with every class for F2 and B2 plus plain rows
    (so lanes that stop early share a wave with lanes that run to the end), on the
    frame SISO in both recursion layouts, the row SISO (siso<0, 4>; ragged at 790)
    and the state-per-lane prototype (float32 only: tdec_api.hip siso_route), with
    f32 and f64 channel LLRs, sf 0.7 and 1.0."""
    _assert_siso_classes(n)
    if kernel.startswith("frame"):
        monkeypatch.setenv("TDEC_FR_SISO_WPD1_MAX", "100000" if kernel == "frame-one" else "0")
    elif kernel == "row":
        monkeypatch.setenv("TDEC_SISO_FRAME", "0")
    else:
        monkeypatch.setenv("TDEC_SISO_SPL", "1")
    for f64 in ((False,) if kernel == "spl" else (False, True)):
        for sf in (0.7, 1.0):
            _check_siso(n, f64, sf)


@pytest.mark.parametrize("n", SISO_N)
@pytest.mark.parametrize("layout", ["one", "two"])
def test_siso_every_depth_class_logmap_frame(n, layout, monkeypatch):
    """The log-MAP frame SISO (the same segment rounds) on the same batch, f32 and
    f64 channel LLRs, sf 0.7 and 1.0."""
    _assert_siso_classes(n, algo=1)
    monkeypatch.setenv("TDEC_FR_SISO_WPD1_MAX", "100000" if layout == "one" else "0")
    for f64 in (False, True):
        for sf in (0.7, 1.0):
            _check_siso(n, f64, sf, algo=1)


# ---- decode level ----------------------------------------------------------------------

def _oracle_args(c):
    return (c.N, c.punct["period"], T.puncture_matrix(c.punct), c.iterations, c.perm, c.inv_perm, TAB)


def _late(n, d):
    return F.depth_class(n, int(d)) in ("c", "d")


def _assert_decode_classes(c, llr, late_rows, b_row, algo=0):
    """late_rows: every SISO 1 and SISO 2 call, in each direction, of each row is in
    class (c) or (d) in iteration 1 and in a later iteration (max-log; log-MAP: at
    least one call of each decoder and direction, and one past iteration 1).
    b_row: decoder 1's B2 is in class (b) in iteration 1 and in a later one."""
    n = c.N
    for r in late_rows:
        d = O.decode_depths(llr[r], *_oracle_args(c), algo)
        late = np.vectorize(lambda x: _late(n, x))(d)
        if algo == 0:
            assert late.all(), (r, d.tolist())
        else:
            assert late.any(axis=0).all() and late[1:].any(), (r, d.tolist())
    if b_row is not None and algo == 0:
        d = O.decode_depths(llr[b_row], *_oracle_args(c))
        assert F.depth_class(n, int(d[0, 0, 1])) == "b"
        assert any(F.depth_class(n, int(d[it, 0, 1])) == "b" for it in range(1, c.iterations))


@functools.lru_cache(maxsize=None)
def _batch3(n, rate, algo):
    c = M.DVBRCS2_Turbo(n, rate, algo="log-map" if algo else "max-log")
    llr = F.decode_batch3(c)
    ref = O.decode_batch(llr, *_oracle_args(c), algo=algo, want_lfinal=True, nthreads=8)
    for x in (llr, *ref):
        x.setflags(write=False)
    return c, llr, ref


@functools.lru_cache(maxsize=None)
def _batch69(n, rate, algo):
    c = M.DVBRCS2_Turbo(n, rate, algo="log-map" if algo else "max-log")
    llr = F.decode_batch69(c)
    ref = O.decode_batch(llr, *_oracle_args(c), algo=algo, want_lfinal=True, nthreads=16)
    for x in (llr, *ref):
        x.setflags(write=False)
    return c, llr, ref


def _equal(bits, lf, ref):
    np.testing.assert_array_equal(bits, ref[0])
    np.testing.assert_array_equal(lf, ref[1])


@pytest.mark.parametrize("n,rate", DECODE_SHAPES)
@pytest.mark.parametrize("decoder", ["frame-one", "frame-two", "lowlat"])
def test_decode_three_codewords(n, rate, decoder, monkeypatch):
    """B = 3 (never, class (b), plain) on the frame decoder in both recursion
    layouts -- a chain in which no segment merges in any round, in every SISO of
    every iteration -- and on the low-latency decoder (TDEC_FRAME=0), whose pass 2
    then rewrites its whole store."""
    c, llr, ref = _batch3(n, rate, 0)
    _assert_decode_classes(c, llr, [0], 1)
    if decoder == "lowlat":
        monkeypatch.setenv("TDEC_FRAME", "0")
    else:
        monkeypatch.setenv("TDEC_FR_WPD1_MAX", "100000" if decoder == "frame-one" else "0")
    bits, lf = c.decode_batch(llr, return_lfinal=True)
    _equal(bits, lf, ref)


def _decode_planes(c, llr, n_iter=False):
    B = llr.shape[0]
    c.reserve(70_000)          # a handle reserved for a large batch decodes small ones per lane
    dev = torch.device("cuda", 0)
    bits = torch.empty((B, c.k_info), dtype=torch.int32, device=dev)
    lf = torch.empty((B, c.k_info), dtype=torch.float64, device=dev)
    nit = torch.zeros(B, dtype=torch.int32, device=dev) if n_iter else None
    planes = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device=dev)
    c.depuncture_device(torch.from_numpy(np.array(llr)).to(dev), planes)
    c.decode_planes_device(planes, B, bits, lf, n_iter=nit)
    torch.cuda.synchronize()
    return (bits.cpu().numpy(), lf.cpu().numpy()) + ((nit.cpu().numpy(),) if n_iter else ())


@pytest.mark.parametrize("n,rate", DECODE_SHAPES)
def test_decode_throughput_tile(n, rate):
    """The throughput tile decoder (siso8), 64 + 5 codewords: never-merging rows in
    lanes 0, 31 and 63 of the full tile and lane 2 of the partial one, a class (b)
    row (B2 just past the ring) in lane 1, plain rows everywhere else, so lanes that
    stop at the first checkpoints sit beside lanes that run F2 and B2 to the end."""
    c, llr, ref = _batch69(n, rate, 0)
    _assert_decode_classes(c, llr, F.TILE_LATE_LANES, F.TILE_B_LANE)
    bits, lf = _decode_planes(c, llr)
    _equal(bits, lf, ref)


@pytest.mark.parametrize("n,rate", DECODE_SHAPES)
def test_decode_logmap_frame(n, rate):
    """The log-MAP frame decoder (the same segment machinery) on the same 69 rows."""
    c, llr, ref = _batch69(n, rate, 1)
    _assert_decode_classes(c, llr, F.TILE_LATE_LANES, None, algo=1)
    bits, lf = c.decode_batch(llr, return_lfinal=True)
    _equal(bits, lf, ref)


@functools.lru_cache(maxsize=None)
def _es_ref(n, rate):
    c, llr, _ = _batch69(n, rate, 0)
    ref = R.decode_early_stop_batch(llr, c.N, c.punct, c.iterations, c.perm, c.inv_perm, TAB)
    for x in ref:
        x.setflags(write=False)
    return ref


@pytest.mark.parametrize("n,rate", DECODE_SHAPES)
@pytest.mark.parametrize("es_decoder", ["frame", "tile"])
def test_decode_early_stop(n, rate, es_decoder):
    """early_stop=True on the same 69 rows, frame decoder and tile decoder: n_iter and
    every row equal the restated rule (tests/early_stop_ref.py).  The rows' SISOs are
    the fixed decode's, so their classes are those asserted from decode_depths for
    the iterations that run."""
    c0, llr, _ = _batch69(n, rate, 0)
    _assert_decode_classes(c0, llr, F.TILE_LATE_LANES, F.TILE_B_LANE)
    ref = _es_ref(n, rate)
    c = M.DVBRCS2_Turbo(n, rate, early_stop=True, es_decoder=es_decoder)
    if es_decoder == "tile":
        bits, lf, nit = _decode_planes(c, llr, n_iter=True)
    else:
        bits, lf, nit = c.decode_batch(llr, return_lfinal=True, return_iters=True)
    np.testing.assert_array_equal(nit, ref[2])
    _equal(bits, lf, ref)
