"""The workload generator's kernels (tdec_workload.hip: k_workload, k_workload_fading,
k_workload_faded, k_workload_frame, k_workload_frame_branches, k_count_errors) on the designed cases of
tests/generator_cases.py, through the C ABI and modulations_amd/workload.py.

Bit for bit: everything without a transcendental -- the info bits, the coded bits, the labels, the error
counts, the top-tail samples (u1 = 1: the table point, or los; u2 = 1: the imaginary part untouched) and
the fading product h x given the device's gains.  Noise and gains: per component
    |device - ref64| <= ulp32(y_ref) / 2 + 4 tau rad_ref
(generator_cases: ref64 the float64 Box-Muller of the float32 uniforms and the float32 sigma, rad_ref
its radius, the half ulp the final float32 addition), on all 130 rows of every case: two full tiles and
a partial one, at cw0 = 0, 2^32 - 40 (the carry into counter word 1 inside a tile), 2^40 + 12345 and
2^63 - 200, with seeds below 2^32, 0xDEADBEEF12345 and 2^64 - 1.

tau, measured on the host from the float32 restatement (test_generator_cases_host.py): 2.25e-7, so the
bound is 9.0e-7 of the radius.  Worst on the MI355X, over the 262 checks of this file: an excess over the
half ulp of 2.2e-7 of the radius (a noise sample in a tile of the tail family), a quarter of the bound; the
rotation is the restatement's bit for bit (0 ulp); the variance ratios are 0.992 .. 1.002 against 4
standard errors of 0.02 (BPSK) .. 0.06 (256QAM).  Each test prints its figures (`-s`).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fading_ref as F  # noqa: E402
import generator_abi as GA  # noqa: E402
import generator_cases as G  # noqa: E402
import pilot_csi_ref as P  # noqa: E402
from oracle import workload_ref as WR  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

_KEEP = {}
C128 = np.complex128


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _codec(n, rate):
    if (n, rate) not in _KEEP:
        _KEEP[n, rate] = M.DVBRCS2_Turbo(n, rate)
    return _KEEP[n, rate]


def _handle(n, rate):
    """A handle for any N with generator_cases.made_up_perm, as generator_abi._env builds its N = 50 one."""
    if ("h", n, rate) not in _KEEP:
        c = _codec(48, "1/3")
        perm = G.made_up_perm(n)
        _KEEP["h", n, rate] = M._Handle(0, n, T.PUNCTURE_PATTERNS[rate], 8, 0, perm, np.argsort(perm).astype(np.int32),
                                        T.packed_tables(c.next_state, c.out_W, c.out_Y, c.prev_state, c.prev_input))
    return _KEEP["h", n, rate]


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _sigma(n0):
    return float(np.sqrt(n0 / 2))


def _check(what, dev, y_ref, rad):
    e = G.excess(dev, y_ref, rad)
    print(f"{what}: worst excess / rad {np.max(e):.3e} (bound {G.bound():.3e})")
    assert np.all(e <= G.bound()), what


def _clean(c, mod, seed, cw0, Bn=G.B):
    """The table points of the batch: the sigma = 0 run (the mapper family checks them against the oracle)."""
    return _np(W.make_symbols(c, Bn, mod, float("inf"), seed, "cuda", cw0=cw0, want_info=False)[1])


# ---- counter family -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cw0,seed", G.COUNTERS, ids=G.COUNTER_IDS)
def test_info_bits_on_every_row(cw0, seed):
    for n in (48, 212):
        got = _np(W.info_bits(_codec(n, "1/3"), G.B, seed, "cuda", cw0=cw0))
        assert np.array_equal(got, WR.info_bits(G.cws(cw0, G.B), n, seed))


@pytest.mark.parametrize("cw0,seed", G.COUNTERS, ids=G.COUNTER_IDS)
def test_noise_on_every_row(cw0, seed):
    k = G.BULK
    c = _codec(k["n"], k["rate"])
    info, syms, n0 = W.make_symbols(c, G.B, k["mod"], k["ebn0"], seed, "cuda", cw0=cw0)
    assert np.array_equal(_np(info), WR.info_bits(G.cws(cw0, G.B), k["n"], seed))
    x = _clean(c, k["mod"], seed, cw0)
    ref, rad = G.noise(G.cws(cw0, G.B), k["S"], seed, _sigma(n0))
    _check("noise", _np(syms), x.astype(C128) + ref, rad)


@pytest.mark.parametrize("cw0,seed", G.COUNTERS, ids=G.COUNTER_IDS)
def test_gains_and_branch_noise_on_every_row(cw0, seed):
    k = G.BULK
    c, S, coh, R = _codec(k["n"], k["rate"]), k["S"], k["coh"], k["R"]
    cw, nh = G.cws(cw0, G.B), -(-k["S"] // k["coh"])
    x = _clean(c, k["mod"], seed, cw0)
    one = {"K": k["K"], "coh": coh}
    _, y1, n0, h1 = W.make_symbols(c, G.B, k["mod"], k["ebn0"], seed, "cuda", cw0=cw0, want_info=False, fading=one)
    _, yb, _, hb = W.make_symbols(c, G.B, k["mod"], k["ebn0"], seed, "cuda", cw0=cw0, want_info=False,
                                  fading={**one, "branches": R})
    y1, h1, yb, hb = _np(y1), _np(h1), _np(yb), _np(hb)
    assert np.array_equal(yb[:, 0], y1) and np.array_equal(hb[:, 0], h1)
    for b in range(R):
        ref, rad = G.gains(cw, nh, seed, k["K"], b)
        _check(f"gains of branch {b}", hb[:, b], ref, rad)
        n_ref, n_rad = G.noise(cw, S, seed, _sigma(n0), G.NOISE, b)
        hx = G.fade32(hb[:, b][:, G.block_of(S, coh)], x)
        _check(f"h x + n of branch {b}", yb[:, b], hx.astype(C128) + n_ref, n_rad)


@pytest.mark.parametrize("cw0,seed", G.COUNTERS, ids=G.COUNTER_IDS)
def test_frames_pilot_noise_and_rotation(cw0, seed):
    k, fr = G.BULK, G.FRAME
    c, S = _codec(k["n"], k["rate"]), k["S"]
    lay = D.PilotLayout(fr["plen"], fr["dlen"])
    ppos, p = lay.pilot_positions(S), lay.pilots(S)
    cw = G.cws(cw0, G.B)
    for R in (1, 3):
        fading = {"K": k["K"], "coh": k["coh"], "branches": R}
        gen = lambda cfo: W.make_symbols(c, G.B, k["mod"], fr["ebn0"], seed, "cuda", cw0=cw0, want_info=False,  # noqa: E731
                                         fading=fading, pilots=lay, cfo=cfo)
        _, f0, n0, h0 = gen(0.0)
        f0, h0 = _np(f0), _np(h0)
        assert f0.shape == (G.B, R, lay.frame_len(S))
        # the data positions copy the unframed symbols, and h_true there is their gain
        _, y, n0y, g = W.make_symbols(c, G.B, k["mod"], fr["ebn0"], seed, "cuda", cw0=cw0, want_info=False, fading=fading)
        dpos = lay.data_positions(S)
        assert n0y == n0 and np.array_equal(f0[:, :, dpos], _np(y))
        assert np.array_equal(h0[:, :, dpos], _np(g)[:, :, G.block_of(S, k["coh"])])
        for b in range(R):
            hp = G.pilot32(h0[:, b][:, ppos], p[None, :])
            ref, rad = G.noise(cw, len(p), seed, _sigma(n0), G.PILOT, b)
            assert np.array_equal(ref, P.pilot_noise(cw, len(p), seed, _sigma(n0), b))
            _check(f"pilots of branch {b} of {R}", f0[:, b][:, ppos], hp.astype(C128) + ref, rad)
        _, f1, _, h1 = gen(fr["cfo"])
        fg = P.cfo_of(cw, seed, fr["cfo"])
        for got, base in ((_np(f1), f0), (_np(h1), h0)):
            for b in range(R):
                ref = P.rotate(base[:, b], fg).view(np.float32)
                g = np.ascontiguousarray(got[:, b]).view(np.float32)
                worst = np.max(np.abs(g.astype(np.float64) - ref) / np.spacing(np.maximum(np.abs(ref), np.abs(g))))
                print("max |device - restatement| in ulp", worst)
                assert worst <= 1.0
        assert not np.array_equal(_np(f1), f0)
    # branch 0 of the branch call is the single-branch call
    _, s0, _, hs = W.make_symbols(c, G.B, k["mod"], fr["ebn0"], seed, "cuda", cw0=cw0, want_info=False,
                                  fading={"K": k["K"], "coh": k["coh"]}, pilots=lay, cfo=fr["cfo"])
    assert np.array_equal(_np(s0), _np(f1)[:, 0]) and np.array_equal(_np(hs), _np(h1)[:, 0])


@pytest.mark.parametrize("cw0,seed", G.COUNTERS, ids=G.COUNTER_IDS)
def test_error_counts_on_every_row(cw0, seed):
    """k_count_errors forms cw0 + row itself: one flipped bit per row of the reference info bits counts 1
    on every row, the carry into counter word 1 and both upper words included; the device's own info bits
    count 0."""
    c = _codec(G.BULK["n"], G.BULK["rate"])
    dec = torch.from_numpy(G.counter_decoded(cw0, seed)).cuda()
    assert np.array_equal(_np(W.count_errors(c, dec, seed, cw0=cw0)), np.ones(G.B, np.int32))
    own = W.info_bits(c, G.B, seed, "cuda", cw0=cw0).to(torch.int32).contiguous()
    assert not _np(W.count_errors(c, own, seed, cw0=cw0)).any()


# ---- tail family --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.TAILS, ids=G.TAIL_IDS)
def test_tail_draws(row):
    dom, off, s, role, v = row
    k = G.BULK
    c, lane = _codec(k["n"], k["rate"]), G.TAIL_LANE
    cw0 = G.TAIL_CW0 + off - lane
    cw = G.cws(cw0, 64)
    x = _clean(c, k["mod"], G.TAIL_SEED, cw0, 64)
    if dom == "noise":
        _, syms, n0 = W.make_symbols(c, 64, k["mod"], k["ebn0"], G.TAIL_SEED, "cuda", cw0=cw0, want_info=False)
        dev = _np(syms)
        ref, rad = G.noise(cw, k["S"], G.TAIL_SEED, _sigma(n0))
        y_ref, point = x.astype(C128) + ref, x
    else:
        _, _, _, h = W.make_symbols(c, 64, k["mod"], k["ebn0"], G.TAIL_SEED, "cuda", cw0=cw0, want_info=False,
                                    fading={"K": G.TAIL_K, "coh": 1})
        dev = _np(h)
        y_ref, rad = G.gains(cw, k["S"], G.TAIL_SEED, G.TAIL_K)
        point = np.full(dev.shape, F.los_scat(G.TAIL_K)[0], np.complex64)
    _check("the tile of the tail draw", dev, y_ref, rad)
    one = (slice(lane, lane + 1), slice(s, s + 1))
    print("device", dev[one], "reference", y_ref[one], "point", point[one])
    assert G.tail_ok(row, dev[one], y_ref[one], rad[one], point[one])


# ---- mapper family ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rate,bps", G.MAPPER, ids=G.MAPPER_IDS)
def test_mapper_labels_coded_bits_and_info_bits(n, rate, bps):
    h, Bn = _handle(n, rate), G.MAPPER_B
    cw0, seed = G.CW0S[2], G.SEEDS[1]
    S = -(-h.enc_len // bps)
    tab = G.label_table(bps)
    syms = torch.full((Bn, S), np.nan, dtype=torch.complex64, device="cuda")
    info = torch.full((Bn, 2 * n), 7, dtype=torch.uint8, device="cuda")
    iq = np.ascontiguousarray(tab).view(np.float32)
    h.call("tdec_workload_dev", Bn, cw0, seed, N.ptr(iq), 1 << bps, bps, 0.0,
           N.ptr(syms), N.ptr(info), None)
    want_info = WR.info_bits(G.cws(cw0, Bn), n, seed)
    assert np.array_equal(_np(info), want_info)
    only = torch.full((Bn, 2 * n), 7, dtype=torch.uint8, device="cuda")
    h.call("tdec_info_bits_dev", Bn, cw0, seed, N.ptr(only), None)
    assert np.array_equal(_np(only), want_info)
    coded = G.encode_rows(want_info, n, rate)
    assert coded.shape == (Bn, h.enc_len)
    got = _np(syms)
    lab = G.labels(coded, bps)
    assert np.array_equal(got.real, lab) and np.array_equal(got.imag, -lab)
    out = torch.full((Bn, h.enc_len), 7, dtype=torch.uint8, device="cuda")
    h.call("tdec_encode_dev", Bn, N.ptr(torch.from_numpy(want_info).cuda()), N.ptr(out), None)
    assert np.array_equal(_np(out), coded)


# ---- fading family ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,coh,R", [(K, coh, None) for K, coh in G.FADING_ONE] + G.FADING_BRANCHES)
def test_fading_gains_and_products(K, coh, R):
    f = G.FADING
    c, S, Bn, seed, cw0 = _codec(f["n"], f["rate"]), f["S"], f["B"], f["seed"], f["cw0"]
    cw, nh = G.cws(cw0, Bn), -(-S // coh)
    fading = {"K": K, "coh": coh} if R is None else {"K": K, "coh": coh, "branches": R}
    x = _clean(c, f["mod"], seed, cw0, Bn)
    assert x.shape == (Bn, S)
    _, y, n0, h = W.make_symbols(c, Bn, f["mod"], f["ebn0"], seed, "cuda", cw0=cw0, want_info=False, fading=fading)
    _, y0, _, hc = W.make_symbols(c, Bn, f["mod"], float("inf"), seed, "cuda", cw0=cw0, want_info=False, fading=fading)
    y, h, y0, hc = (_np(t).reshape(Bn, R or 1, -1) for t in (y, h, y0, hc))
    assert np.array_equal(h, hc) and h.shape == (Bn, R or 1, nh)
    blk = G.block_of(S, coh)
    for b in range(R or 1):
        ref, rad = G.gains(cw, nh, seed, K, b)
        _check(f"gains of branch {b}", h[:, b], ref, rad)
        hx = G.fade32(h[:, b][:, blk], x)
        assert np.array_equal(y0[:, b], hx)                            # the clean part, bit for bit
        n_ref, n_rad = G.noise(cw, S, seed, _sigma(n0), G.NOISE, b)
        _check(f"h x + n of branch {b}", y[:, b], hx.astype(C128) + n_ref, n_rad)


# ---- variance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", list(D.MODULATIONS))
def test_noise_variance_is_n0_over_two(mod):
    v = G.VARIANCE
    c = _codec(v["n"], v["rate"])
    _, syms, n0 = W.make_symbols(c, G.B, mod, v["ebn0"], v["seed"], "cuda", cw0=v["cw0"], want_info=False)
    assert n0 == W.noise_n0(D.constellation(mod), 1 / 3, D.MODULATIONS[mod]["bps"], v["ebn0"])
    noise = _np(syms).astype(C128) - _clean(c, mod, v["seed"], v["cw0"])
    x = np.concatenate([noise.real.ravel(), noise.imag.ravel()])
    assert x.size == G.B * syms.shape[1] * 2
    print(mod, "variance per dimension / (N0 / 2)", np.mean(x * x) / (n0 / 2), "over", x.size)
    assert G.variance_ok(x, n0)


# ---- error counts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.COUNT_N)
def test_error_counts(n):
    h = _handle(n, "1/3")
    for cw0, dec, want in G.count_batches(n):
        errs = torch.full((len(dec),), -5, dtype=torch.int32, device="cuda")
        h.call("tdec_count_errors_dev", len(dec), cw0, G.COUNT_SEED, N.ptr(torch.from_numpy(dec).cuda()), N.ptr(errs), None)
        assert np.array_equal(_np(errs), want)


def test_count_errors_wrapper_at_the_largest_counter():
    c = _codec(48, "1/3")
    cw0, dec, want = G.count_batches(48)[0]
    got = W.count_errors(c, torch.from_numpy(dec).cuda(), G.COUNT_SEED, cw0=cw0)
    assert np.array_equal(_np(got), want)


# ---- ABI ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call,case", GA.params("tdec_count_errors_dev"))
def test_generator_abi_refusals(call, case):
    GA.check(call, case)
