"""Early termination on the throughput tile decoder (csrc/tdec_kernels.hip
k_turbo_decode_es / k_turbo_decode_logmap_es, tdec_decode_*_es_tile*).
Every max-log row is compared with IEEE == on bits, L_final and n_iter against the
numpy restatement of the rule (tests/early_stop_ref.py); log-MAP rows against the
product's own fixed decode with iterations = n_iter[row], and their n_iter against
the frame decoder's."""
import ctypes as C
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import early_stop_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402

TAB, _ = O.trellis()
I = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tile(n, rate, iters=I, **kw):
    kw.setdefault("interleaver", "valid-perm")
    return M.DVBRCS2_Turbo(n, rate, iters, early_stop=True, es_decoder="tile", **kw)


def _ref(c, llr):
    return R.decode_early_stop_batch(llr, c.N, c.punct, c.iterations, c.perm, c.inv_perm, TAB)


def _equal(got, ref):
    bits, lf, nit = got
    np.testing.assert_array_equal(nit, ref[2])
    assert np.array_equal(bits, ref[0])
    np.testing.assert_array_equal(lf, ref[1])


def _check_host(c, llr, ref):
    bits, lf, nit = c.decode_batch(llr, return_lfinal=True, return_iters=True)
    assert nit.dtype == np.int32 and nit.shape == (llr.shape[0],)
    _equal((bits, lf, nit), ref)


def _check_device(c, llr, ref, planes=False):
    B = llr.shape[0]
    d = torch.tensor(llr, device="cuda")
    bits = torch.zeros((B, c.k_info), dtype=torch.int32, device="cuda")
    lf = torch.zeros((B, c.k_info), dtype=torch.float64, device="cuda")
    nit = torch.zeros(B, dtype=torch.int32, device="cuda")
    if planes:
        c.reserve(B)
        pl = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
        c.depuncture_device(d, pl)
        c.decode_planes_device(pl, B, bits, lfinal=lf, n_iter=nit)
    else:
        c.decode_device(d, bits=bits, lfinal=lf, n_iter=nit)
    torch.cuda.synchronize()
    _equal((bits.cpu().numpy(), lf.cpu().numpy(), nit.cpu().numpy()), ref)


@pytest.fixture(scope="module")
def mixed48():
    """N = 48 r = 1/3 valid-perm, 64 rows at 0 dB: one tile whose lanes end on different
    trips; row 62 all zeros, row 63 noise-free +-20.  (codec, llr, reference), shared
    and unchanged."""
    c = _tile(48, "1/3")
    info, llr = R.bpsk_llrs(c, np.random.default_rng(48), 64, 0.0)
    llr[62] = 0.0
    llr[63] = ((1 - 2.0 * c.encode(info[63])) * 20.0).astype(np.float32)
    llr.setflags(write=False)
    ref = _ref(c, llr)
    for x in ref:
        x.setflags(write=False)
    return c, llr, ref


def test_one_tile_host_pointers(mixed48):
    c, llr, ref = mixed48
    assert len(set(ref[2].tolist())) >= 3 and ref[2].min() == 2 and ref[2].max() == I
    _check_host(c, llr, ref)
    one = c.decode(llr[5])
    assert np.array_equal(one, ref[0][5])


@pytest.mark.parametrize("planes", [False, True])
def test_one_tile_device_pointers(mixed48, planes):
    c, llr, ref = mixed48
    _check_device(c, llr, ref, planes)


def test_lfinal_and_n_iter_are_optional(mixed48):
    c, llr, ref = mixed48
    assert np.array_equal(c.decode_batch(llr), ref[0])
    bits = c.decode_device(torch.tensor(llr, device="cuda"))
    assert np.array_equal(bits.cpu().numpy(), ref[0])


def test_partial_tile_and_lane_placement(mixed48):
    c, llr, ref = mixed48
    rows = (np.arange(69) * 7) % 64
    big = np.ascontiguousarray(llr[rows])
    want = tuple(x[rows] for x in ref)
    _check_host(c, big, want)
    _check_device(c, big, want)
    _check_host(c, llr[9:10], tuple(x[9:10] for x in ref))


@pytest.mark.parametrize("cap", ["1", "2", None])
def test_several_tiles_per_wave(mixed48, cap, monkeypatch):
    """B = 320: five tiles, tile t the fixture rows rolled by 13 t.  One wave takes all
    five from the queue (resetting its lane state each time), two waves share them, or
    every tile has its own wave."""
    c, llr, ref = mixed48
    rows = np.concatenate([np.roll(np.arange(64), 13 * t) for t in range(5)])
    big = np.ascontiguousarray(llr[rows])
    want = tuple(x[rows] for x in ref)
    if cap is None:
        monkeypatch.delenv("TDEC_ES_TILE_WAVES", raising=False)
    else:
        monkeypatch.setenv("TDEC_ES_TILE_WAVES", cap)
    _check_device(c, big, want)
    _check_device(c, big, want, planes=True)


@pytest.mark.parametrize("n,rate,interleaver,B,ebn0", [
    (48, "1/3", "reference", 16, 2.0),
    (212, "1/2", "valid-perm", 8, 2.0),
    (212, "1/2", "reference", 4, 4.0),     # runs to the cap
    (752, "1/3", "valid-perm", 4, 1.5),
    (848, "1/3", "valid-perm", 2, 1.5),    # beyond the frame decoder's LDS plan
])
def test_block_sizes_and_interleavers(n, rate, interleaver, B, ebn0):
    c = _tile(n, rate, interleaver=interleaver, inv_perm="stable")
    _, llr = R.bpsk_llrs(c, np.random.default_rng(n + B), B, ebn0)
    ref = _ref(c, llr)
    if (n, interleaver) == (212, "reference"):
        assert (ref[2] == I).all()
    _check_host(c, llr, ref)
    _check_device(c, llr, ref)


@pytest.mark.parametrize("iters", [1, 2])
def test_edge_iteration_counts(mixed48, iters):
    _, llr, _ = mixed48
    c = _tile(48, "1/3", iters)
    ref = _ref(c, llr[:16])
    assert (ref[2] == iters).all()
    _check_host(c, llr[:16], ref)
    _check_device(c, llr[:16], ref)
    if iters == 1:   # the plain one-iteration decode
        pb, pl = M.DVBRCS2_Turbo(48, "1/3", 1, interleaver="valid-perm").decode_batch(llr[:16], return_lfinal=True)
        assert np.array_equal(pb, ref[0])
        np.testing.assert_array_equal(pl, ref[1])


def test_nan_and_inf_rows_decide_zero():
    """Plain `<`: a NaN total decides 0 in the rule as in the reference's output."""
    c = _tile(48, "1/3")
    _, llr = R.bpsk_llrs(c, np.random.default_rng(7), 4, 2.0)
    llr[0, ::7] = np.nan
    llr[1, :] = np.nan
    llr[2, ::5] = np.inf
    llr[3, ::3] = -0.0
    _check_host(c, llr, _ref(c, llr))


@pytest.mark.parametrize("n,rate,B,ebn0", [(48, "1/3", 32, 0.0), (212, "1/2", 8, 1.5)])
def test_logmap_rows_equal_the_fixed_decode_with_their_count(n, rate, B, ebn0):
    c = _tile(n, rate, algo="log-map")
    _, llr = R.bpsk_llrs(c, np.random.default_rng(n), B, ebn0)
    bits, lf, nit = c.decode_batch(llr, return_lfinal=True, return_iters=True)
    assert nit.min() >= 2 and nit.max() <= I
    for k in sorted(set(nit.tolist())):
        rows = np.flatnonzero(nit == k)
        fixed = M.DVBRCS2_Turbo(n, rate, k, algo="log-map", interleaver="valid-perm")
        fb, fl = fixed.decode_batch(llr[rows], return_lfinal=True)
        assert np.array_equal(bits[rows], fb), k
        np.testing.assert_array_equal(lf[rows], fl)
    frame = M.DVBRCS2_Turbo(n, rate, I, algo="log-map", interleaver="valid-perm", early_stop=True)
    np.testing.assert_array_equal(nit, frame.decode_batch(llr, return_iters=True)[1])


def test_host_pointer_chunks(mixed48, monkeypatch):
    """B = 130 through tdec_decode_batch_es_tile in chunks of 33 rows (three whole chunks
    and one of 31): bits, L_final and n_iter equal those of the same call in one chunk,
    the numpy rule's, and per count the fixed decode's with iterations = n_iter[row]."""
    c, llr, ref = mixed48
    rows = np.arange(130) % 64
    big = np.ascontiguousarray(llr[rows])
    monkeypatch.delenv("TDEC_HOST_CHUNK", raising=False)
    whole = c.decode_batch(big, return_lfinal=True, return_iters=True)
    monkeypatch.setenv("TDEC_HOST_CHUNK", "33")
    bits, lf, nit = c.decode_batch(big, return_lfinal=True, return_iters=True)
    monkeypatch.delenv("TDEC_HOST_CHUNK")
    _equal((bits, lf, nit), whole)
    _equal((bits, lf, nit), tuple(x[rows] for x in ref))
    assert len(set(nit.tolist())) >= 3
    for k in sorted(set(nit.tolist())):
        at = np.flatnonzero(nit == k)
        fb, fl = M.DVBRCS2_Turbo(48, "1/3", k, interleaver="valid-perm").decode_batch(big[at], return_lfinal=True)
        assert np.array_equal(bits[at], fb), k
        np.testing.assert_array_equal(lf[at], fl)


def test_runs_without_the_frame_decoder(mixed48, monkeypatch):
    _, llr, ref = mixed48
    monkeypatch.setenv("TDEC_FRAME", "0")
    c = _tile(48, "1/3")   # constructs, and decodes on the tile kernel
    _check_host(c, llr, ref)
    _check_device(c, llr, ref)


def test_frame_and_tile_agree(mixed48):
    c, llr, _ = mixed48
    frame = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm", early_stop=True)
    f = frame.decode_batch(llr, return_lfinal=True, return_iters=True)
    t = c.decode_batch(llr, return_lfinal=True, return_iters=True)
    for a, b in zip(f, t):
        np.testing.assert_array_equal(a, b)


def test_ber_sweep_on_the_tile_decoder(tmp_path):
    from modulations_amd import ber
    base = ["--mod", "QPSK", "--n", "48", "--rate", "1/3", "--interleaver", "valid-perm", "--ebn0", "1",
            "--codewords", "192", "--batch", "128", "--seed", "5", "--early-stop"]
    out_t, out_f = tmp_path / "tile.json", tmp_path / "frame.json"
    tile_args = base + ["--es-decoder", "tile", "--out", str(out_t)]
    rt, = ber.main(tile_args)
    rf, = ber.main(base + ["--out", str(out_f)])
    for k in ("bit_errors", "frame_errors", "iter_hist", "codewords"):
        assert rt[k] == rf[k], k
    assert sum(rt["iter_hist"]) == 192
    doc = json.loads(out_t.read_text())
    assert doc["config"]["es_decoder"] == "tile" and doc["points"][0]["es_decoder"] == "tile"
    assert "es_decoder" not in json.loads(out_f.read_text())["config"]
    # the other decoder into the same file is another sweep, both ways
    with pytest.raises(SystemExit):
        ber.main(base + ["--out", str(out_t)])
    with pytest.raises(SystemExit):
        ber.main(base + ["--es-decoder", "tile", "--out", str(out_f)])


def test_capacity_is_an_error_and_writes_nothing(mixed48):
    """A _dev call above tdec_reserve: TDEC_ECAPACITY through the ABI, outputs untouched."""
    _, llr, _ = mixed48
    c = _tile(48, "1/3")
    c.reserve(64)
    B = 128
    L, h = M._n.lib(), c.handle.h
    d = torch.tensor(np.ascontiguousarray(llr[np.arange(B) % 64]), device="cuda")
    bits = torch.full((B, c.k_info), 7, dtype=torch.int32, device="cuda")
    lf = torch.full((B, c.k_info), 7.0, dtype=torch.float64, device="cuda")
    nit = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    pl = torch.zeros(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.tdec_decode_batch_es_tile_dev(h, B, d.data_ptr(), d.shape[1], bits.data_ptr(), lf.data_ptr(),
                                         nit.data_ptr(), st)
    assert rc == M._n.TDEC_ECAPACITY
    rc = L.tdec_decode_planes_es_tile_dev(h, B, pl.data_ptr(), bits.data_ptr(), lf.data_ptr(), nit.data_ptr(), st)
    assert rc == M._n.TDEC_ECAPACITY
    torch.cuda.synchronize()
    assert (bits == 7).all() and (lf == 7.0).all() and (nit == 7).all()
