"""Early termination with finished lanes refilled (csrc/tdec_kernels.hip
k_turbo_decode_refill / k_turbo_decode_logmap_refill, tdec_decode_*_es_refill*;
DESIGN.md §8.3).  Every max-log row is compared with IEEE == on bits, L_final and
n_iter against the numpy restatement of the rule (tests/early_stop_ref.py); log-MAP
rows against the product's own fixed decode with iterations = n_iter[row], and their
n_iter against the frame decoder's.  With one persistent wave the launch's trip count
(tdec_es_refill_stats) must equal the schedule model of test_early_stop_refill_host."""
import ctypes as C
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import early_stop_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from test_early_stop_refill_host import refill_schedule  # noqa: E402

TAB, _ = O.trellis()
I = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _refill(n, rate, iters=I, **kw):
    kw.setdefault("interleaver", "valid-perm")
    return M.DVBRCS2_Turbo(n, rate, iters, early_stop=True, es_decoder="refill", **kw)


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


def _run_device(c, llr, planes=False):
    """One _dev call; the output tensors start from a sentinel no decode produces."""
    B = llr.shape[0]
    d = torch.tensor(llr, device="cuda")
    bits = torch.full((B, c.k_info), 7, dtype=torch.int32, device="cuda")
    lf = torch.full((B, c.k_info), np.nan, dtype=torch.float64, device="cuda")
    nit = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    if planes:
        c.reserve(B)
        pl = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
        c.depuncture_device(d, pl)
        c.decode_planes_device(pl, B, bits, lfinal=lf, n_iter=nit)
    else:
        c.decode_device(d, bits=bits, lfinal=lf, n_iter=nit)
    return bits, lf, nit


def _check_device(c, llr, ref, planes=False):
    out = _run_device(c, llr, planes)
    torch.cuda.synchronize()
    _equal(tuple(x.cpu().numpy() for x in out), ref)


@pytest.fixture(scope="module")
def mixed48():
    """N = 48 r = 1/3 valid-perm, 64 rows at 0 dB whose codewords end on different
    iterations; row 62 all zeros, row 63 noise-free +-20 (the fixture of
    test_gpu_early_stop_tile.py).  (codec, llr, reference), shared and unchanged."""
    c = _refill(48, "1/3")
    info, llr = R.bpsk_llrs(c, np.random.default_rng(48), 64, 0.0)
    llr[62] = 0.0
    llr[63] = ((1 - 2.0 * c.encode(info[63])) * 20.0).astype(np.float32)
    llr.setflags(write=False)
    ref = _ref(c, llr)
    for x in ref:
        x.setflags(write=False)
    # a condition on the input, by the numpy rule: lanes end on at least three different trips
    assert len(set(ref[2].tolist())) >= 3 and ref[2].min() == 2 and ref[2].max() == I
    return c, llr, ref


def _rows(mixed48, rows):
    _, llr, ref = mixed48
    rows = np.asarray(rows)
    return np.ascontiguousarray(llr[rows]), tuple(x[rows] for x in ref)


ROLLED = np.concatenate([np.roll(np.arange(64), 13 * t) for t in range(5)])   # B = 320, as test_several_tiles_per_wave


# 1 ---- one wave, no refill ------------------------------------------------------------------
def test_one_tile_host_pointers(mixed48):
    c, llr, ref = mixed48
    _check_host(c, llr, ref)
    assert c.refill_stats() == (int(ref[2].max()), 64)   # 64 lanes filled once, the slowest row's trips
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


# 2 ---- refills into mixed lanes, one wave --------------------------------------------------
def test_one_wave_refills_mixed_lanes(mixed48, monkeypatch):
    """B = 320 on one wave: lanes end on different trips and each takes the next row
    while its neighbours are mid-decode.  The trip count is the documented schedule's,
    below what whole tiles cost: no alias of the tile decoder passes this."""
    c, _, _ = mixed48
    big, want = _rows(mixed48, ROLLED)
    monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    model = refill_schedule(want[2])
    tile_trips = sum(int(want[2][i:i + 64].max()) for i in range(0, 320, 64))
    assert tile_trips == 40 and model[1] == 320 and model[0] < tile_trips
    for planes in (False, True):
        _check_device(c, big, want, planes)
        assert c.refill_stats() == model


# 3 ---- several waves ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap", ["2", None])
def test_several_waves(mixed48, cap, monkeypatch):
    c, _, _ = mixed48
    big, want = _rows(mixed48, ROLLED)
    if cap is None:
        monkeypatch.delenv("TDEC_ES_TILE_WAVES", raising=False)
    else:
        monkeypatch.setenv("TDEC_ES_TILE_WAVES", cap)
    waves = 5 if cap is None else int(cap)   # one wave per 64 rows at most
    for planes in (False, True):
        _check_device(c, big, want, planes)
        trips, refills = c.refill_stats()
        assert refills == 320
        # whichever rows a wave is handed, it runs no longer than one wave that takes them all
        assert int(want[2].max()) <= trips <= refill_schedule(want[2])[0] * waves


# 4 ---- partial last claim and idle lanes -----------------------------------------------------
def test_partial_claims_and_idle_lanes(mixed48, monkeypatch):
    c, llr, ref = mixed48
    big, want = _rows(mixed48, (np.arange(69) * 7) % 64)
    _check_host(c, big, want)
    _check_device(c, big, want)
    _check_host(c, llr[9:10], tuple(x[9:10] for x in ref))        # B = 1: 63 lanes idle from the start
    _check_device(c, llr[9:10], tuple(x[9:10] for x in ref), planes=True)
    assert c.refill_stats() == (int(ref[2][9]), 1)
    monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    _check_device(c, big, want)                                     # 69 rows on one wave
    assert c.refill_stats() == refill_schedule(want[2])
    # B = 65 with row 64 the slowest: the first lane to end takes it, the other 63 stay done
    order = np.argsort(ref[2], kind="stable")
    big, want = _rows(mixed48, np.concatenate([order, order[-1:]]))
    _check_device(c, big, want)
    assert c.refill_stats() == (int(ref[2].min() + ref[2].max()), 65)


# 5 ---- clustered stragglers ---------------------------------------------------------------------
@pytest.mark.parametrize("slow_first", [True, False])
def test_clustered_stragglers(mixed48, slow_first, monkeypatch):
    """64 copies of a row that runs to the cap and 128 fast rows, one wave: refills while
    most of the wave is at a high iteration index, and the cap firing on different trips
    in different lanes.  (The all-zero row is no straggler: its decisions repeat at once,
    so the rule gives it 2 iterations; it is one of the fast rows here, and the slow row
    is the fixture's first that the rule runs to the cap.)"""
    c, _, ref = mixed48
    assert ref[2][62] == 2 == ref[2].min()
    fast = np.flatnonzero(ref[2] == 2)
    assert 62 in fast and 63 in fast
    fast = fast[np.arange(128) % len(fast)]
    slow = np.full(64, np.flatnonzero(ref[2] == I)[0])
    big, want = _rows(mixed48, np.concatenate([slow, fast] if slow_first else [fast, slow]))
    monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    _check_device(c, big, want)
    assert c.refill_stats() == refill_schedule(want[2])
    _check_device(c, big, want, planes=True)


# 6 ---- blocks and interleavers -----------------------------------------------------------------
@pytest.mark.parametrize("n,rate,interleaver,B,ebn0", [
    (48, "1/3", "reference", 16, 2.0),
    (212, "1/2", "valid-perm", 8, 2.0),     # N % 8 != 0: the ragged instantiation
    (752, "1/3", "valid-perm", 4, 1.5),
    (848, "1/3", "valid-perm", 4, 1.5),     # beyond the frame decoder's LDS plan
    (64, "1/2", "valid-perm", 70, 2.0),     # one previous-decision row pair exactly, a refill of 6 rows
])
def test_block_sizes_and_interleavers(n, rate, interleaver, B, ebn0, monkeypatch):
    c = _refill(n, rate, interleaver=interleaver, inv_perm="stable")
    _, llr = R.bpsk_llrs(c, np.random.default_rng(n + B), B, ebn0)
    ref = _ref(c, llr)
    _check_device(c, llr, ref)
    if B > 64:
        monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    _check_device(c, llr, ref, planes=True)
    assert c.refill_stats() == refill_schedule(ref[2])


# 7 ---- iteration caps of 1 and 2 --------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 2])
def test_edge_iteration_counts(mixed48, iters, monkeypatch):
    big, _ = _rows(mixed48, np.arange(80) % 64)
    c = _refill(48, "1/3", iters)
    ref = _ref(c, big)
    assert (ref[2] == iters).all()
    _check_host(c, big[:16], tuple(x[:16] for x in ref))
    monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    _check_device(c, big, ref)
    assert c.refill_stats() == (2 * iters, 80)
    if iters == 1:   # the plain one-iteration decode
        pb, pl = M.DVBRCS2_Turbo(48, "1/3", 1, interleaver="valid-perm").decode_batch(big, return_lfinal=True)
        assert np.array_equal(pb, ref[0])
        np.testing.assert_array_equal(pl, ref[1])


# 8 ---- non-finite rows ---------------------------------------------------------------------------
def test_nan_and_inf_rows_decide_zero(mixed48, monkeypatch):
    """Plain `<`: a NaN total decides 0 in the rule as in the reference's output; the
    rows beside them, and the rows that later take their lanes, are undisturbed."""
    c = _refill(48, "1/3")
    _, llr = R.bpsk_llrs(c, np.random.default_rng(7), 4, 2.0)
    llr[0, ::7] = np.nan
    llr[1, :] = np.nan
    llr[2, ::5] = np.inf
    llr[3, ::3] = -0.0
    ref = _ref(c, llr)
    _check_host(c, llr, ref)
    _check_device(c, llr, ref)
    # 128 rows on one wave, the four rows alternating with four of the fixture's: every lane
    # that held one of them is refilled, and every one of them lands in a used lane
    _, fix, fref = mixed48
    rows = np.arange(128)
    odd = rows % 8 < 4
    big = np.where(odd[:, None], llr[rows % 4], fix[rows % 64]).astype(np.float32)
    want = tuple(np.where(odd.reshape((-1,) + (1,) * (a.ndim - 1)), a[rows % 4], b[rows % 64])
                 for a, b in zip(ref, fref))
    monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    _check_device(c, np.ascontiguousarray(big), want)
    assert c.refill_stats() == refill_schedule(want[2])


# 9 ---- log-MAP -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rate,B,ebn0", [(48, "1/3", 32, 0.0), (212, "1/2", 8, 1.5)])
def test_logmap_rows_equal_the_fixed_decode_with_their_count(n, rate, B, ebn0, monkeypatch):
    c = _refill(n, rate, algo="log-map")
    _, llr = R.bpsk_llrs(c, np.random.default_rng(n), B, ebn0)
    llr = np.ascontiguousarray(np.concatenate([llr, llr, llr[::-1]]))   # 3 B rows: refills on one wave at N = 48
    monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    bits, lf, nit = c.decode_batch(llr, return_lfinal=True, return_iters=True)
    assert nit.min() >= 2 and nit.max() <= I
    assert c.refill_stats() == refill_schedule(nit)
    for k in sorted(set(nit.tolist())):
        rows = np.flatnonzero(nit == k)
        fixed = M.DVBRCS2_Turbo(n, rate, k, algo="log-map", interleaver="valid-perm")
        fb, fl = fixed.decode_batch(llr[rows], return_lfinal=True)
        assert np.array_equal(bits[rows], fb), k
        np.testing.assert_array_equal(lf[rows], fl)
    frame = M.DVBRCS2_Turbo(n, rate, I, algo="log-map", interleaver="valid-perm", early_stop=True)
    np.testing.assert_array_equal(nit, frame.decode_batch(llr, return_iters=True)[1])


# 10 ---- host-pointer chunks ---------------------------------------------------------------------
def test_host_pointer_chunks(mixed48, monkeypatch):
    """B = 130 through tdec_decode_batch_es_refill in chunks of 33 rows (three whole
    chunks and one of 31)."""
    c, _, _ = mixed48
    big, want = _rows(mixed48, np.arange(130) % 64)
    monkeypatch.setenv("TDEC_HOST_CHUNK", "33")
    _check_host(c, big, want)
    assert c.refill_stats() == (int(want[2][99:].max()), 31)   # the last launch: the chunk of 31
    monkeypatch.delenv("TDEC_HOST_CHUNK")
    _check_host(c, big, want)


# 11 ---- without the frame decoder -------------------------------------------------------------
def test_runs_without_the_frame_decoder(mixed48, monkeypatch):
    _, llr, ref = mixed48
    monkeypatch.setenv("TDEC_FRAME", "0")
    c = _refill(48, "1/3")   # constructs, and decodes on the refill kernel
    _check_host(c, llr, ref)
    _check_device(c, llr, ref)


# 12 ---- the three early-stop decoders agree -------------------------------------------------
def test_frame_tile_and_refill_agree(mixed48):
    c, _, _ = mixed48
    big, _ = _rows(mixed48, ROLLED[:200])
    frame = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm", early_stop=True)
    tile = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm", early_stop=True, es_decoder="tile")
    f = frame.decode_batch(big, return_lfinal=True, return_iters=True)
    t = tile.decode_batch(big, return_lfinal=True, return_iters=True)
    r = c.decode_batch(big, return_lfinal=True, return_iters=True)
    for a, b, d in zip(f, t, r):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, d)


# 13 ---- capacity ---------------------------------------------------------------------------------
def test_capacity_is_an_error_and_writes_nothing(mixed48):
    """A _dev call above tdec_reserve_es_refill: TDEC_ECAPACITY through the ABI, outputs
    untouched.  tdec_reserve alone does not size the per-wave plane buffers."""
    _, llr, _ = mixed48
    B = 128
    d = torch.tensor(np.ascontiguousarray(llr[np.arange(B) % 64]), device="cuda")
    bits = torch.full((B, 96), 7, dtype=torch.int32, device="cuda")
    lf = torch.full((B, 96), 7.0, dtype=torch.float64, device="cuda")
    nit = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = M._n.lib()
    for reserve in ("tdec_reserve_es_refill", "tdec_reserve"):
        c = _refill(48, "1/3")
        h = c.handle.h
        # (tdec_reserve: for the whole batch, and still no plane buffers for this mode)
        assert getattr(L, reserve)(h, 64 if reserve == "tdec_reserve_es_refill" else B) == 0
        pl = torch.zeros(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
        rc = L.tdec_decode_batch_es_refill_dev(h, B, d.data_ptr(), d.shape[1], bits.data_ptr(), lf.data_ptr(),
                                               nit.data_ptr(), st)
        assert rc == M._n.TDEC_ECAPACITY, reserve
        rc = L.tdec_decode_planes_es_refill_dev(h, B, pl.data_ptr(), bits.data_ptr(), lf.data_ptr(), nit.data_ptr(), st)
        assert rc == M._n.TDEC_ECAPACITY, reserve
        torch.cuda.synchronize()
        assert (bits == 7).all() and (lf == 7.0).all() and (nit == 7).all()
        assert c.refill_stats() == (0, 0)   # nothing was launched


# 14 ---- reuse ---------------------------------------------------------------------------------------
def test_back_to_back_calls_on_one_handle(mixed48, monkeypatch):
    """Two _dev calls on one handle and stream with nothing between them: the row queue
    and the statistics start from zero in each launch."""
    c, _, _ = mixed48
    a, want_a = _rows(mixed48, ROLLED[:200])
    b, want_b = _rows(mixed48, ROLLED[::-1][:90])
    monkeypatch.setenv("TDEC_ES_TILE_WAVES", "1")
    c.reserve(200)
    out_a = _run_device(c, a)
    out_b = _run_device(c, b)
    torch.cuda.synchronize()
    _equal(tuple(x.cpu().numpy() for x in out_a), want_a)
    _equal(tuple(x.cpu().numpy() for x in out_b), want_b)
    assert c.refill_stats() == refill_schedule(want_b[2])


# 15 ---- the BER tool -----------------------------------------------------------------------------
def test_ber_sweep_on_the_refill_decoder(tmp_path):
    from modulations_amd import ber
    base = ["--mod", "QPSK", "--n", "48", "--rate", "1/3", "--interleaver", "valid-perm", "--ebn0", "0,1",
            "--codewords", "320", "--batch", "192", "--seed", "5", "--early-stop"]
    out_r, out_t = tmp_path / "refill.json", tmp_path / "tile.json"
    rr = ber.main(base + ["--es-decoder", "refill", "--out", str(out_r)])
    rt = ber.main(base + ["--es-decoder", "tile", "--out", str(out_t)])
    assert len(rr) == len(rt) == 2
    for a, b in zip(rr, rt):
        for k in ("bit_errors", "frame_errors", "iter_hist", "codewords"):
            assert a[k] == b[k], k
        assert sum(a["iter_hist"]) == 320 and a["es_decoder"] == "refill"
    doc = json.loads(out_r.read_text())
    assert doc["config"]["es_decoder"] == "refill" and doc["points"][0]["es_decoder"] == "refill"
    with pytest.raises(SystemExit):   # the other decoder into the same file is another sweep
        ber.main(base + ["--es-decoder", "tile", "--out", str(out_r)])
