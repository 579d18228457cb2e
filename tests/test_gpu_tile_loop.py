"""The persistent tile loop of the fixed-iteration decoders (turbo_decode_tiles behind
k_turbo_decode / k_turbo_decode_logmap) with several tiles per wave, bit for bit.

A wave takes a second tile only when a batch has more tiles than the device has resident
waves (about 2 048 on an MI355X), and the tile queue is handed out only from four tiles
per wave, so no test-sized batch reaches either on its own.  TDEC_TILE_WAVES (read per
call, tdec_api.hip tile_queue()) caps the persistent waves of one launch.  With it the
ten tiles of B = 581 (nine full tiles and one of 5 rows) are served

  cap "1", "2"   from the queue (10 >= 4 x waves): nxt = n_waves + atomicAdd(...)
  cap "3"        by static striding, 3 to 4 tiles per wave: nxt = tile + n_waves
  unset          one tile per wave

and the three tiles of B = 133 with cap "1" by static striding on a single wave.

The rows are the 69 of tests/codec_matrix.py (an all-zero and a saturating row among
them): tile t holds the first 64 rolled by 13 t, the partial tile rows 64..68, so every
tile differs from every other and a row changes its lane from tile to tile.  A wave that
carried anything from one tile to the next -- Le2 instead of the zero a-priori at it = 0,
a stale checkpoint, a per-lane output pointer -- gives other bits.  The reference is the
fixture's own oracle decode, indexed; outputs start from sentinels (bits 7, L_final NaN),
so a tile nobody served shows too.  Every comparison is IEEE ==; no tolerance.

Block sizes: decode_kernel() picks the ragged kernel by N % win_of(algo).  Max-log
(WIN_ML = 8) is ragged at N = 212 (212 % 8 = 4) and even at 48 and 64.  For log-MAP
(WIN_LM = 2) no block size of the tables is ragged, so its ragged kernel has no case
here.  N = 48 lies below the beta ring, and its last chunk of the epilogue has kn = 16.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("trans_tables")]

import codec_matrix as CM  # noqa: E402
from oracle import oracle as O  # noqa: E402
from modulations_amd import _native as NT  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from test_gpu_codec_matrix import B_BIG, _equal, _outputs, _strided  # noqa: E402

CAP = "TDEC_TILE_WAVES"
CODECS = [(48, "1/3"), (64, "3/4"), (212, "1/2")]
CASES = [(n, rate, algo) for n, rate in CODECS for algo in CM.ALGOS]
CASE_IDS = [f"{CM.codec_id(n, rate)}-{algo}" for n, rate, algo in CASES]
# (B, cap): ten tiles through the queue, by static striding and one per wave; three tiles on one wave
LOADS = [(581, "1"), (581, "2"), (581, "3"), (581, None), (133, "1")]
LOAD_IDS = [f"B{b}-cap{c or 'unset'}" for b, c in LOADS]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def tile_rows(B):
    """Fixture row of each of the B rows: full tile t = rows 0..63 rolled by 13 t, then rows 64.."""
    full, tail = divmod(B, 64)
    assert full <= 9 and tail <= CM.ROWS - 64
    return np.concatenate([np.roll(np.arange(64), 13 * t) for t in range(full)] + [64 + np.arange(tail)])


def _set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv(CAP, raising=False)
    else:
        monkeypatch.setenv(CAP, cap)


@functools.lru_cache(maxsize=None)
def _iter_ref(n, rate, algo, iters, prims):
    punct = T.PUNCTURE_PATTERNS[rate]
    perm, inv = CM.interleaver(n, "reference")
    bits, lf = O.decode_batch(CM.fixed_batch(n, rate)[1], n, punct["period"], T.puncture_matrix(punct), iters,
                              perm, inv, CM.TAB, algo=CM.ALGOS.index(algo), want_lfinal=True)
    bits.setflags(write=False)
    lf.setflags(write=False)
    return bits, lf


def ref_of(n, rate, algo, iters=CM.ITERATIONS):
    """(bits, L_final) of the 69 fixture rows by the oracle (codec_matrix's own for 8 iterations)."""
    if iters == CM.ITERATIONS:
        return CM.fixed_ref(n, rate, algo)
    return _iter_ref(n, rate, algo, iters, algo != "max-log" and O.trans_pinned())


@pytest.fixture(scope="module")
def reserved():
    """As test_gpu_codec_matrix.reserved: handles reserved for B_BIG only, so they have no
    small-batch workspace and every batch runs the tile kernel.  One per (N, rate, algorithm,
    iterations)."""
    cache = {}

    def get(n, rate, algo, iters=CM.ITERATIONS):
        key = (n, rate, algo, iters)
        if key not in cache:
            c = cache[key] = M.DVBRCS2_Turbo(n, rate, iters, algo=algo, inv_perm="stable")
            c.reserve(B_BIG)
        c = cache[key]
        assert c.early_stop_capacity() == 0, "the small-batch workspace exists: not the tile route any more"
        return c

    yield get
    cache.clear()


def _decode_planes(c, llr, lfinal=True):
    B = llr.shape[0]
    bits, lf = _outputs(c, B)
    planes = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
    c.depuncture_device(torch.tensor(llr, device="cuda"), planes)
    c.decode_planes_device(planes, B, bits, lf if lfinal else None)
    torch.cuda.synchronize()
    return bits.cpu().numpy(), lf.cpu().numpy()


def _check(c, n, rate, algo, B, lfinal=True, iters=CM.ITERATIONS):
    rows = tile_rows(B)
    llr = np.ascontiguousarray(CM.fixed_batch(n, rate)[1][rows])
    ref = ref_of(n, rate, algo, iters)
    bits, lf = _decode_planes(c, llr, lfinal)
    if lfinal:
        _equal(bits, lf, (ref[0][rows], ref[1][rows]))
    else:
        assert bits.dtype == np.int32 and np.array_equal(bits, ref[0][rows])
        assert np.isnan(lf).all()   # the sentinel: nothing was written


def test_tiles_differ():
    """What the module relies on: every row of B = 581 sits in another lane in every tile, and
    the tiles' references differ (a tile decoded twice, or skipped, cannot pass)."""
    rows = tile_rows(581)
    assert rows.shape == (581,) and sorted(set(rows.tolist())) == list(range(CM.ROWS))
    lanes = {}
    for i, r in enumerate(rows):
        lanes.setdefault(int(r), []).append(i % 64)
    assert all(len(v) == len(set(v)) for v in lanes.values())
    for n, rate, algo in CASES:
        ref = ref_of(n, rate, algo)[1][rows[:576]].reshape(9, 64, -1)
        for a in range(9):
            for b in range(a):
                assert not np.array_equal(ref[a], ref[b])


@pytest.mark.parametrize("lfinal", [True, False], ids=["lfinal", "bits-only"])
@pytest.mark.parametrize("B,cap", LOADS, ids=LOAD_IDS)
@pytest.mark.parametrize("n,rate,algo", CASES, ids=CASE_IDS)
def test_planes(n, rate, algo, B, cap, lfinal, reserved, monkeypatch):
    _set_cap(monkeypatch, cap)
    _check(reserved(n, rate, algo), n, rate, algo, B, lfinal)
    reserved(n, rate, algo)   # still no small-batch workspace


def test_planes_n752_two_waves(reserved, monkeypatch):
    """The benchmark's block size, five tiles per wave from the queue."""
    _set_cap(monkeypatch, "2")
    _check(reserved(752, "1/3", "max-log"), 752, "1/3", "max-log", 581)


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("B,cap", LOADS, ids=LOAD_IDS)
@pytest.mark.parametrize("algo", CM.ALGOS)
def test_edge_iteration_counts(algo, B, cap, iters, reserved, monkeypatch):
    """A wave's next tile starts at it = 0 with the zero a-priori (p.aux), not with the Le2 the
    previous tile left; with one iteration it = 0 is also the last (sf = 1.0, Le1 stored)."""
    _set_cap(monkeypatch, cap)
    _check(reserved(48, "1/3", algo, iters), 48, "1/3", algo, B, iters=iters)


def test_strided_rows_one_wave(reserved, monkeypatch):
    """tdec_decode_batch_dev (de-puncture into the handle's planes, then the tile route) on rows
    with a stride longer than the walk and NaN in between, all ten tiles on one wave."""
    n, rate, algo = 212, "1/2", "max-log"
    _set_cap(monkeypatch, "1")
    c = reserved(n, rate, algo)
    rows = tile_rows(581)
    d = _strided(np.ascontiguousarray(CM.fixed_batch(n, rate)[1][rows]))
    bits, lf = _outputs(c, len(rows))
    c.handle.call("tdec_decode_batch_dev", len(rows), NT.ptr(d), d.stride(0), NT.ptr(bits), NT.ptr(lf),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = ref_of(n, rate, algo)
    _equal(bits.cpu().numpy(), lf.cpu().numpy(), (ref[0][rows], ref[1][rows]))
    reserved(n, rate, algo)


def test_host_pointer_two_waves(monkeypatch):
    """decode_batch (tdec_decode_batch) ends in the same tile route.  A log-MAP handle with
    TDEC_FRAME=0 has no small-batch decoder, so its 581 rows run k_turbo_decode_logmap."""
    n, rate, algo = 212, "1/2", "log-map"
    monkeypatch.setenv("TDEC_FRAME", "0")
    _set_cap(monkeypatch, "2")
    rows = tile_rows(581)
    c = M.DVBRCS2_Turbo(n, rate, CM.ITERATIONS, algo=algo, inv_perm="stable")
    ref = ref_of(n, rate, algo)
    _equal(*c.decode_batch(CM.fixed_batch(n, rate)[1][rows], return_lfinal=True), (ref[0][rows], ref[1][rows]))
