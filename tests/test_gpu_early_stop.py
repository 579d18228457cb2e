"""Early termination on the frame decoder (csrc/tdec_frame.hip k_turbo_decode_frame_es,
tdec_decode_*_es).  Every max-log row is compared with IEEE == on
bits, L_final and n_iter against the numpy restatement of the rule
(tests/early_stop_ref.py, itself pinned to the oracle's fixed-iteration decode by
tests/test_early_stop_rule.py); log-MAP rows against the product's own fixed decode
with iterations = n_iter[row]."""
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


def _ref(c, llr, iters=None):
    return R.decode_early_stop_batch(llr, c.N, c.punct, c.iterations if iters is None else iters, c.perm, c.inv_perm,
                                     TAB)


def _check_host(c, llr, ref):
    bits, lf, nit = c.decode_batch(llr, return_lfinal=True, return_iters=True)
    assert nit.dtype == np.int32 and nit.shape == (llr.shape[0],)
    np.testing.assert_array_equal(nit, ref[2])
    assert np.array_equal(bits, ref[0])
    np.testing.assert_array_equal(lf, ref[1])


def _check_device(c, llr, ref, planes=False):
    B = llr.shape[0]
    d = torch.tensor(llr, device="cuda")
    bits = torch.zeros((B, c.k_info), dtype=torch.int32, device="cuda")
    lf = torch.zeros((B, c.k_info), dtype=torch.float64, device="cuda")
    nit = torch.zeros(B, dtype=torch.int32, device="cuda")
    if planes:
        pl = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
        c.depuncture_device(d, pl)
        c.decode_planes_device(pl, B, bits, lfinal=lf, n_iter=nit)
    else:
        c.decode_device(d, bits=bits, lfinal=lf, n_iter=nit)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(nit.cpu().numpy(), ref[2])
    assert np.array_equal(bits.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(lf.cpu().numpy(), ref[1])


@pytest.fixture(scope="module")
def mixed48():
    """N = 48 r = 1/3 valid-perm, 64 rows at 0 dB: mixed iteration counts; row 62 all
    zeros, row 63 noise-free +-20.  (codec, llr, reference), shared and unchanged."""
    c = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm", early_stop=True)
    info, llr = R.bpsk_llrs(c, np.random.default_rng(48), 64, 0.0)
    llr[62] = 0.0
    llr[63] = ((1 - 2.0 * c.encode(info[63])) * 20.0).astype(np.float32)
    llr.setflags(write=False)
    return c, llr, _ref(c, llr)


def test_mixed_counts_host_pointers(mixed48):
    c, llr, ref = mixed48
    assert len(set(ref[2].tolist())) >= 3 and ref[2].min() == 2 and ref[2].max() == I
    _check_host(c, llr, ref)
    one = c.decode(llr[5])   # decode() of one frame takes the same path
    assert np.array_equal(one, ref[0][5])


@pytest.mark.parametrize("planes", [False, True])
def test_mixed_counts_device_pointers(mixed48, planes):
    c, llr, ref = mixed48
    _check_device(c, llr, ref, planes)


def test_n_iter_is_optional(mixed48):
    c, llr, ref = mixed48
    assert np.array_equal(c.decode_batch(llr), ref[0])
    bits = c.decode_device(torch.tensor(llr, device="cuda"))
    assert np.array_equal(bits.cpu().numpy(), ref[0])


@pytest.mark.parametrize("n,rate,interleaver,B,ebn0", [
    (48, "1/3", "reference", 16, 2.0),
    (212, "1/2", "valid-perm", 8, 2.0),
    (212, "1/2", "reference", 4, 4.0),     # runs to the cap
    (752, "1/3", "valid-perm", 4, 1.5),    # two waves per recursion direction
    (848, "1/3", "valid-perm", 2, 1.5),    # Le2 in global scratch
])
def test_block_sizes_and_interleavers(n, rate, interleaver, B, ebn0):
    c = M.DVBRCS2_Turbo(n, rate, I, interleaver=interleaver, inv_perm="stable", early_stop=True)
    _, llr = R.bpsk_llrs(c, np.random.default_rng(n + B), B, ebn0)
    ref = _ref(c, llr)
    if (n, interleaver) == (212, "reference"):
        assert (ref[2] == I).all()
    _check_host(c, llr, ref)
    _check_device(c, llr, ref)


@pytest.mark.parametrize("layout", ["one", "two"])
@pytest.mark.parametrize("n", [212, 848])
def test_both_recursion_layouts(n, layout, monkeypatch):
    """One wave per recursion direction and two, whatever fr_wpd would pick."""
    monkeypatch.setenv("TDEC_FR_WPD1_MAX", "100000" if layout == "one" else "0")
    c = M.DVBRCS2_Turbo(n, "1/3", I, interleaver="valid-perm", early_stop=True)
    _, llr = R.bpsk_llrs(c, np.random.default_rng(n), 3, 2.0)
    _check_host(c, llr, _ref(c, llr))


@pytest.mark.parametrize("iters", [1, 2])
def test_edge_iteration_counts(mixed48, iters):
    _, llr, _ = mixed48
    c = M.DVBRCS2_Turbo(48, "1/3", iters, interleaver="valid-perm", early_stop=True)
    ref = _ref(c, llr[:16])
    assert (ref[2] == iters).all()
    _check_host(c, llr[:16], ref)
    _check_device(c, llr[:16], ref)


def test_nan_and_inf_rows_decide_zero():
    """Plain `<`: a NaN total decides 0 in the rule as in the reference's output."""
    c = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm", early_stop=True)
    _, llr = R.bpsk_llrs(c, np.random.default_rng(7), 4, 2.0)
    llr[0, ::7] = np.nan
    llr[1, :] = np.nan
    llr[2, ::5] = np.inf
    llr[3, ::3] = -0.0
    _check_host(c, llr, _ref(c, llr))


def test_chunks(mixed48):
    """One row more than a launch takes: the rows on both sides of the chunk boundary
    equal the same rows decoded alone (and every row equals the reference)."""
    _, llr, ref = mixed48
    c = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm", early_stop=True)
    c.reserve(64)
    cap = c.early_stop_capacity()
    assert 0 < cap <= 64 and cap % 64 == 0
    B = cap + 1
    rows = np.arange(B) % 64
    big = np.ascontiguousarray(llr[rows])
    want = tuple(x[rows] for x in ref)
    _check_device(c, big, want)
    _check_device(c, big, want, planes=True)
    assert c.early_stop_capacity() == cap   # the calls chunked; they did not regrow the workspace
    for r in (cap - 1, cap):
        alone = c.decode_batch(big[r:r + 1], return_lfinal=True, return_iters=True)
        for a, w in zip(alone, want):
            np.testing.assert_array_equal(a[0], w[r])


def test_host_pointer_chunks(mixed48, monkeypatch):
    c, llr, ref = mixed48
    rows = np.arange(100) % 64
    big = np.ascontiguousarray(llr[rows])
    monkeypatch.setenv("TDEC_HOST_CHUNK", "33")
    _check_host(c, big, tuple(x[rows] for x in ref))


@pytest.mark.parametrize("n,rate,B,ebn0", [(48, "1/3", 32, 0.0), (212, "1/2", 8, 1.5)])
def test_logmap_rows_equal_the_fixed_decode_with_their_count(n, rate, B, ebn0):
    c = M.DVBRCS2_Turbo(n, rate, I, algo="log-map", interleaver="valid-perm", early_stop=True)
    _, llr = R.bpsk_llrs(c, np.random.default_rng(n), B, ebn0)
    bits, lf, nit = c.decode_batch(llr, return_lfinal=True, return_iters=True)
    assert nit.min() >= 2 and nit.max() <= I
    for k in sorted(set(nit.tolist())):
        rows = np.flatnonzero(nit == k)
        fixed = M.DVBRCS2_Turbo(n, rate, k, algo="log-map", interleaver="valid-perm")
        fb, fl = fixed.decode_batch(llr[rows], return_lfinal=True)
        assert np.array_equal(bits[rows], fb), k
        np.testing.assert_array_equal(lf[rows], fl)


def test_early_stop_false_is_the_plain_decoder(mixed48):
    _, llr, _ = mixed48
    plain = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm")
    off = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm", early_stop=False)
    pb, pl = plain.decode_batch(llr, return_lfinal=True)
    ob, ol, it = off.decode_batch(llr, return_lfinal=True, return_iters=True)
    assert np.array_equal(pb, ob) and (it == I).all()
    np.testing.assert_array_equal(pl, ol)
    d = torch.tensor(llr, device="cuda")
    assert torch.equal(plain.decode_device(d), off.decode_device(d))
    with pytest.raises(ValueError):
        off.decode_device(d, n_iter=torch.zeros(64, dtype=torch.int32, device="cuda"))


def test_unavailable_frame_decoder_is_an_error(mixed48, monkeypatch):
    c, llr, _ = mixed48
    c.handle   # created while the frame decoder is available
    monkeypatch.setenv("TDEC_FRAME", "0")
    with pytest.raises(ValueError, match="frame decoder"):
        c.decode_batch(llr)
    out = np.zeros(c.k_info, np.int32)
    rc = M._n.lib().tdec_decode_batch_es(c.handle.h, 1, llr.ctypes.data, llr.shape[1], out.ctypes.data, None, None)
    assert rc == M._n.TDEC_EUNSUPPORTED and b"TDEC_FRAME" in M._n.lib().tdec_last_error()


def test_ber_sweep_records_iterations(tmp_path):
    """python -m modulations_amd.ber --early-stop: the counters of a point equal a run of
    the Python API over the same global codewords, and mean_iters matches iter_hist."""
    from modulations_amd import ber
    from modulations_amd.workload import DevicePipeline, count_errors, make_symbols
    out = tmp_path / "es.json"
    args = ["--mod", "QPSK", "--n", "48", "--rate", "1/3", "--interleaver", "valid-perm", "--ebn0", "1",
            "--codewords", "192", "--batch", "128", "--seed", "5", "--early-stop", "--out", str(out)]
    rec, = ber.main(args)
    doc = json.loads(out.read_text())
    assert doc["config"]["early_stop"] is True and doc["points"][0]["iter_hist"] == rec["iter_hist"]
    h = rec["iter_hist"]
    assert len(h) == I + 1 and sum(h) == rec["codewords"] == 192 and h[0] == h[1] == 0
    assert rec["mean_iters"] == sum(i * x for i, x in enumerate(h)) / 192
    dev = torch.device("cuda", 0)
    c = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm", device=0, early_stop=True)
    seed = ber.ebn0_seed(5, 1.0)
    _, syms, n0 = make_symbols(c, 192, "QPSK", 1.0, seed, dev, want_info=False)
    pipe = DevicePipeline(c, "QPSK", 192, dev)
    bits = pipe.run(syms, n0)
    e = count_errors(c, bits, seed)
    assert int(e.sum()) == rec["bit_errors"] and int((e > 0).sum()) == rec["frame_errors"]
    assert torch.bincount(pipe.n_iter, minlength=I + 1).tolist() == h
    # a rerun into the same file without the flag is another sweep
    with pytest.raises(SystemExit):
        ber.main([a for a in args if a != "--early-stop"])
