"""Every codec of the tables on every decoder, bit for bit.

The codec table has 7 block sizes and 4 puncturing rates.  The de-puncture walk,
perm's image, the used-position list, the checkpoint raggedness (N % 8 = 4 at 212
and 220), the short blocks below the beta ring (48, 64) and the LDS plans all depend
on (N, rate), and rates 2/3 and 3/4 never send Y2 and send W2 once a period.  Each
test here is one decoder route, parametrised over all 28 codecs and both algorithms,
on the 69 rows of tests/codec_matrix.py (one full 64-lane tile and a partial one;
an all-zero row and a saturating row beside ordinary ones):

  fixed decode, against oracle.decode_batch
    test_default_route       decode_batch / decode_device on a fresh codec: the frame
                             decoder (at N = 848 with Le2 in global scratch)
    test_frame_off_route     TDEC_FRAME=0: the state-per-lane decoder (max-log); it
                             has no log-MAP form, so log-MAP batches of every size
                             run the tile kernel from the host-pointer entry
    test_tile_planes         a handle reserved for a batch above every routing limit
                             has no small-batch workspace: k_turbo_decode /
                             k_turbo_decode_logmap from de-punctured planes
    test_tile_strided_rows   the same handle, tdec_decode_batch_dev on rows whose
                             stride is longer than the walk, NaN in between
    test_reference_golden    the reference's own decodes (golden/decode_matrix.npz)
                             on the default route and the tile kernel
  early stop, against the restated rule (tests/early_stop_ref.py): bits, L_final, n_iter
    test_early_stop          es_decoder frame / tile / refill, host-pointer and
                             device forms; refill also its trip count
  test_device_encoder        encode_device against the host encoder and the oracle

Every comparison is IEEE == (np.array_equal on bits, assert_array_equal on L_final,
where NaN equals NaN); there is no tolerance in this module.  The references are
computed once per (N, rate, algorithm) by codec_matrix and shared by the routes.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("trans_tables")]

import codec_matrix as CM  # noqa: E402
from conftest import golden  # noqa: E402
from modulations_amd import _native as NT  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from test_early_stop_refill_host import refill_schedule  # noqa: E402

CASES = [(n, rate, algo) for n, rate in CM.CODECS for algo in CM.ALGOS]
CASE_IDS = [f"{CM.codec_id(n, rate)}-{algo}" for n, rate, algo in CASES]
CODEC_IDS = [CM.codec_id(*c) for c in CM.CODECS]
B_BIG = 12_800   # above the small-batch limits (12 288 / 8 192 max-log, 7 168 log-MAP; tdec_api.hip lowlat_max)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _codec(n, rate, algo, **kw):
    return M.DVBRCS2_Turbo(n, rate, CM.ITERATIONS, algo=algo, inv_perm="stable", **kw)


def _equal(bits, lf, ref):
    assert bits.dtype == np.int32 and lf.dtype == np.float64
    assert np.array_equal(bits, ref[0])
    np.testing.assert_array_equal(lf, ref[1])


def _outputs(c, B):
    """Device outputs that start from a sentinel no decode produces."""
    return (torch.full((B, c.k_info), 7, dtype=torch.int32, device="cuda"),
            torch.full((B, c.k_info), np.nan, dtype=torch.float64, device="cuda"))


def _strided(llr):
    """The rows on the device as a view of a wider buffer: stride(0) = walk + 7, NaN between the rows."""
    d = torch.from_numpy(CM.wide(llr)).cuda()[:, :llr.shape[1]]
    assert d.stride(0) == llr.shape[1] + 7 and d.stride(1) == 1
    return d


@pytest.fixture(scope="module")
def reserved():
    """Codecs whose handle was reserved for B_BIG codewords and never for a small
    batch: the small-batch workspace stays unallocated, so every batch size runs
    the throughput tile kernel (tdec_api.hip use_lowlat).  One per (N, rate,
    algorithm), shared by the tile tests and freed with the module."""
    cache = {}

    def get(n, rate, algo):
        key = (n, rate, algo)
        if key not in cache:
            c = cache[key] = _codec(n, rate, algo)
            c.reserve(B_BIG)
        c = cache[key]
        # (the rows the frame decoder's workspace holds: tdec_es_capacity)
        assert c.early_stop_capacity() == 0, "the small-batch workspace exists: not the tile route any more"
        return c

    yield get
    cache.clear()


# ---- fixed decode --------------------------------------------------------------------------
@pytest.mark.parametrize("n,rate,algo", CASES, ids=CASE_IDS)
def test_default_route(n, rate, algo):
    llr = CM.fixed_batch(n, rate)[1]
    ref = CM.fixed_ref(n, rate, algo)
    c = _codec(n, rate, algo)
    assert c.handle.llr_len == llr.shape[1]
    _equal(*c.decode_batch(llr, return_lfinal=True), ref)
    # the device form on the same route, rows with a stride longer than the walk
    bits, lf = _outputs(c, CM.ROWS)
    d = _strided(llr)
    c.decode_device(d, bits=bits, lfinal=lf)
    torch.cuda.synchronize()
    _equal(bits.cpu().numpy(), lf.cpu().numpy(), ref)


@pytest.mark.parametrize("n,rate,algo", CASES, ids=CASE_IDS)
def test_frame_off_route(n, rate, algo, monkeypatch):
    """TDEC_FRAME=0 (read per call).  max-log: the state-per-lane decoder.  log-MAP:
    that decoder has no log-MAP form (lowlat_max is 0), so the host-pointer entry
    runs k_turbo_decode_logmap on the 69 rows."""
    monkeypatch.setenv("TDEC_FRAME", "0")
    assert not NT.lib().tdec_early_stop_available(n)   # the frame decoder is out of the way
    with pytest.raises(ValueError):
        _codec(n, rate, algo, early_stop=True)
    llr = CM.fixed_batch(n, rate)[1]
    _equal(*_codec(n, rate, algo).decode_batch(llr, return_lfinal=True), CM.fixed_ref(n, rate, algo))


def _decode_planes(c, llr):
    B = llr.shape[0]
    bits, lf = _outputs(c, B)
    planes = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
    c.depuncture_device(torch.tensor(llr, device="cuda"), planes)
    c.decode_planes_device(planes, B, bits, lf)   # no reserve(B): the B_BIG workspace
    torch.cuda.synchronize()
    return bits.cpu().numpy(), lf.cpu().numpy()


@pytest.mark.parametrize("n,rate,algo", CASES, ids=CASE_IDS)
def test_tile_planes(n, rate, algo, reserved):
    c = reserved(n, rate, algo)
    _equal(*_decode_planes(c, CM.fixed_batch(n, rate)[1]), CM.fixed_ref(n, rate, algo))
    reserved(n, rate, algo)   # still no small-batch workspace


@pytest.mark.parametrize("n,rate,algo", CASES, ids=CASE_IDS)
def test_tile_strided_rows(n, rate, algo, reserved):
    """tdec_decode_batch_dev through the handle (decode_device would first reserve
    the small-batch workspace for 69 rows and so leave the tile kernel)."""
    c = reserved(n, rate, algo)
    d = _strided(CM.fixed_batch(n, rate)[1])
    bits, lf = _outputs(c, CM.ROWS)
    c.handle.call("tdec_decode_batch_dev", CM.ROWS, NT.ptr(d), d.stride(0), NT.ptr(bits), NT.ptr(lf),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _equal(bits.cpu().numpy(), lf.cpu().numpy(), CM.fixed_ref(n, rate, algo))
    reserved(n, rate, algo)


@pytest.fixture(scope="module")
def G_matrix():
    return golden("decode_matrix")


@pytest.mark.parametrize("n,rate", CM.CODECS, ids=CODEC_IDS)
def test_reference_golden(n, rate, G_matrix, reserved):
    """The reference's own decode() of two codewords per codec (max-log is the only
    algorithm it has): the default route and the tile kernel."""
    key = f"{n}_{rate.replace('/', '_')}"
    llr = G_matrix[f"llr_{key}"]
    ref = G_matrix[f"bits_{key}"], G_matrix[f"lfinal_{key}"]
    c = M.DVBRCS2_Turbo(n, rate, inv_perm=G_matrix[f"inv_{key}"])
    _equal(*c.decode_batch(llr, return_lfinal=True), ref)
    t = reserved(n, rate, "max-log")
    assert np.array_equal(t.inv_perm, G_matrix[f"inv_{key}"])
    _equal(*_decode_planes(t, llr), ref)


# ---- early stop ------------------------------------------------------------------------------
@pytest.mark.parametrize("es", ["frame", "tile", "refill"])
@pytest.mark.parametrize("n,rate,algo", CASES, ids=CASE_IDS)
def test_early_stop(n, rate, algo, es, monkeypatch):
    kw = dict(interleaver="valid-perm", early_stop=True, es_decoder=es)
    llr = CM.early_stop_batch(n, rate)[1]
    ref = CM.early_stop_ref(n, rate, algo)
    assert CM.es_condition(ref[2]), np.bincount(ref[2]).tolist()
    if es == "refill":   # one persistent wave: the documented schedule, so the trip count is known
        monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    c = _codec(n, rate, algo, **kw)
    bits, lf, nit = c.decode_batch(llr, return_lfinal=True, return_iters=True)
    assert nit.dtype == np.int32
    np.testing.assert_array_equal(nit, ref[2])
    _equal(bits, lf, ref)
    if es == "refill":
        assert c.refill_stats() == refill_schedule(ref[2])
    bits, lf = _outputs(c, CM.ROWS)
    nit = torch.full((CM.ROWS,), -1, dtype=torch.int32, device="cuda")
    c.decode_device(torch.tensor(llr, device="cuda"), bits=bits, lfinal=lf, n_iter=nit)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(nit.cpu().numpy(), ref[2])
    _equal(bits.cpu().numpy(), lf.cpu().numpy(), ref)
    if es == "refill":
        assert c.refill_stats() == refill_schedule(ref[2])


# ---- encoder ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rate", CM.CODECS, ids=CODEC_IDS)
def test_device_encoder(n, rate):
    info = CM.fixed_batch(n, rate)[0]
    c = M.DVBRCS2_Turbo(n, rate)
    host = c.encode_batch(info)
    assert np.array_equal(host, CM.oracle_encode(info, n, rate, c.perm))
    out = c.encode_device(torch.from_numpy(info.astype(np.uint8)).cuda())
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), host)
