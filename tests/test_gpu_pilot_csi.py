"""Pilot-aided channel estimation on the device: k_csi_pilots against
its numpy restatement (tests/pilot_csi_ref.py), the fused launch against strip + equalise,
the pipeline against the reference chain, the framing generator, and the estimator's
statistics.  All comparisons are IEEE == with NaN at the same positions."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import early_stop_ref as ES  # noqa: E402
import fading_ref as F  # noqa: E402
import generator_abi as GA  # noqa: E402
import pilot_csi_ref as P  # noqa: E402
from oracle import oracle as O  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

# (S, plen, dlen, B): one symbol; one full segment; one full and one of a single symbol, more
# rows than one wave; a short last segment with an odd plen and an odd row count; S and T odd;
# the longest row (several sweeps of the block over a row)
CASES = [(1, 1, 1, 1), (7, 2, 7, 3), (8, 2, 7, 65), (72, 5, 16, 67), (289, 3, 47, 4), (4512, 4, 564, 2)]
NOISE = ["scalar", "rows", "estimated"]
COMBOS = [(c, m, n) for c in CASES for m in ("linear", "mean") for n in NOISE if not (n == "estimated" and c[1] < 2)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _eq(a, b):
    """IEEE ==, NaN at the same positions."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    ra, rb = a.view(a.real.dtype), b.view(b.real.dtype)
    na, nb = np.isnan(ra), np.isnan(rb)
    return bool(np.array_equal(na, nb) and np.all(ra[~na] == rb[~nb]))


def _teq(a, b):
    return _eq(a.cpu().numpy(), b.cpu().numpy())


_FRAMES = {}


def _frames(case):
    """Random framed bursts for a case (made once): a gain per row that drifts along the
    frame, unit-power data, the layout's pilots, noise of variance 0.05."""
    if case not in _FRAMES:
        S, plen, dlen, B = case
        rng = np.random.default_rng(S * 1000 + plen * 100 + B)
        lay = D.PilotLayout(plen, dlen)
        Tn = lay.frame_len(S)
        cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) * np.sqrt(0.5)  # noqa: E731
        tx = np.empty((B, Tn), np.complex128)
        tx[:, lay.data_positions(S)] = np.exp(2j * np.pi * rng.integers(0, 8, (B, S)) / 8)
        tx[:, lay.pilot_positions(S)] = lay.pilots(S)
        h = cn(B, 1) + cn(B, 1) * np.arange(Tn)[None, :] / Tn
        _FRAMES[case] = (lay, (h * tx + np.sqrt(0.05) * cn(B, Tn)).astype(np.complex64))
    return _FRAMES[case]


def _nv_arg(kind, B, rng):
    if kind == "scalar":
        return 0.0371
    if kind == "rows":
        return 10.0 ** rng.uniform(-3, 1, B)
    return None


def _run(frames, lay, S, nv, mode, floor=0.02, want_nv=True, **kw):
    """estimate_csi_device -> numpy (z, nv_sym, h, nv or None)."""
    B = frames.shape[0]
    dn = torch.from_numpy(nv).cuda() if isinstance(nv, np.ndarray) else nv
    h = torch.empty((B, S), dtype=torch.complex64, device="cuda")
    est = torch.empty(B, dtype=torch.float64, device="cuda") if want_nv and lay.plen >= 2 else None
    z, nvs = D.estimate_csi_device(frames, lay, dn, mode=mode, floor=floor, h_out=h, nv_rows_out=est, **kw)
    assert z.dtype == torch.complex64 and tuple(z.shape) == (B, S)
    assert nvs.dtype == torch.float64 and tuple(nvs.shape) == (B, S)
    return z.cpu().numpy(), nvs.cpu().numpy(), h.cpu().numpy(), None if est is None else est.cpu().numpy()


def _check(got, ref):
    z, nvs, h, est = got
    assert _eq(h, ref["h"])
    assert _eq(z, ref["z"])
    assert _eq(nvs, ref["nv_sym"])
    if est is not None:
        assert _eq(est, ref["nv"])


# ---- the kernel against its restatement --------------------------------------------------------
@pytest.mark.parametrize("case,mode,noise", COMBOS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else v)
def test_kernel_equals_its_numpy_restatement(case, mode, noise):
    S, plen, dlen, B = case
    lay, fr = _frames(case)
    rng = np.random.default_rng(B + S)
    nv = _nv_arg(noise, B, rng)
    floor = 0.02 if noise != "estimated" else 0.051          # some rows' estimates below the floor, some above
    ref = P.estimate(fr, lay.pilots(S), S, plen, dlen, mode=mode, nv=nv, floor=floor)
    if noise == "estimated" and B >= 65:
        assert (ref["nv"] == floor).any() and (ref["nv"] > floor).any()
    _check(_run(torch.from_numpy(fr).cuda(), lay, S, nv, mode, floor=floor), ref)
    # without the optional outputs: the same z and nv_sym
    dn = torch.from_numpy(nv).cuda() if isinstance(nv, np.ndarray) else nv
    z, nvs = D.estimate_csi_device(torch.from_numpy(fr).cuda(), lay, dn, mode=mode, floor=floor)
    assert _eq(z.cpu().numpy(), ref["z"]) and _eq(nvs.cpu().numpy(), ref["nv_sym"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_views_at_odd_offsets_and_rows_alone(case):
    """Frames and outputs one element into their buffers: every output is then 8 modulo 16
    (the vector path with the other slot phase); with only z moved the outputs disagree and
    the scalar path runs.  Then single rows alone (B = 1) against the batch."""
    S, plen, dlen, B = case
    lay, fr = _frames(case)
    noise = "estimated" if plen >= 2 else "scalar"
    nv = _nv_arg(noise, B, None)
    ref = P.estimate(fr, lay.pilots(S), S, plen, dlen, nv=nv)
    Tn = fr.shape[1]
    fbuf = torch.zeros(B * Tn + 1, dtype=torch.complex64, device="cuda")
    fbuf[1:] = torch.from_numpy(fr).cuda().reshape(-1)
    fv = fbuf[1:].view(B, Tn)
    for shift_all in (True, False):
        zb = torch.full((B * S + 1,), np.nan, dtype=torch.complex64, device="cuda")
        nb = torch.full((B * S + 1,), np.nan, dtype=torch.float64, device="cuda")
        hb = torch.full((B * S + 1,), np.nan, dtype=torch.complex64, device="cuda")
        o = 1 if shift_all else 0
        zo, no, ho = zb[1:].view(B, S), nb[o:o + B * S].view(B, S), hb[o:o + B * S].view(B, S)
        r = D.estimate_csi_device(fv, lay, nv, out=zo, nv_out=no, h_out=ho)
        assert r[0] is zo and r[1] is no
        assert _eq(zo.cpu().numpy(), ref["z"]) and _eq(no.cpu().numpy(), ref["nv_sym"]) and _eq(ho.cpu().numpy(), ref["h"])
        assert bool(torch.isnan(zb[0].real)) and bool(torch.isnan(nb[B * S if o == 0 else 0]))   # nothing outside
    full = D.estimate_csi_device(torch.from_numpy(fr).cuda(), lay, nv)
    for r in sorted({0, B // 2, B - 1}):
        one = D.estimate_csi_device(torch.from_numpy(fr[r:r + 1]).cuda(), lay, nv)
        assert _teq(one[0], full[0][r:r + 1]) and _teq(one[1], full[1][r:r + 1])


# ---- non-finite and zero pilots ----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["linear", "mean"])
def test_nonfinite_and_zero_pilots_erase_their_bordering_segments(mode):
    S, plen, dlen, B = 72, 5, 16, 6
    lay, fr = _frames((72, 5, 16, 67))
    fr = fr[:B].copy()
    bs = [lay.block_start(S, j) for j in range(lay.n_blocks(S))]
    fr[0, bs[2] + 1] = np.nan                                # block 2: segments 1 and 2
    fr[1, bs[0]] = np.inf                                    # block 0: segment 0
    fr[2, bs[5] + 4] = -np.inf * 1j                          # block 5, the last: segment 4 (8 symbols)
    fr[3, bs[3]:bs[3] + plen] = 0                            # hp == 0: segments 2 and 3
    fr[4, lay.data_positions(S)[40]] = np.nan                # a data symbol: local
    want = np.zeros((B, S), bool)
    want[0, 16:48] = want[1, 0:16] = want[2, 64:72] = want[3, 32:64] = True
    ref = P.estimate(fr, lay.pilots(S), S, plen, dlen, mode=mode, nv=0.05)
    z, nvs, h, est = _run(torch.from_numpy(fr).cuda(), lay, S, 0.05, mode)
    _check((z, nvs, h, est), ref)
    erased = (z == 0) & np.isposinf(nvs)
    assert np.array_equal(erased, want)
    assert np.isfinite(nvs[~want]).all()
    nan_z = np.isnan(z.real) | np.isnan(z.imag)
    only = np.zeros((B, S), bool)
    only[4, 40] = True
    assert np.array_equal(nan_z, only) and np.isfinite(nvs[4, 40])
    assert np.isnan(est[0]) and np.isnan(est[1]) and np.isnan(est[2]) and np.isfinite(est[3:]).all()
    # the estimate as the noise source: a NaN estimate stays NaN on its row's live symbols
    ref2 = P.estimate(fr, lay.pilots(S), S, plen, dlen, mode=mode, nv=None)
    got2 = _run(torch.from_numpy(fr).cuda(), lay, S, None, mode)
    _check(got2, ref2)
    assert np.array_equal((got2[0] == 0) & np.isposinf(got2[1]), want)
    assert np.isnan(got2[1][0][~want[0]]).all() and np.isfinite(got2[1][3][~want[3]]).all()


# ---- fusion --------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_fused_equals_strip_then_equalise(case, noise):
    S, plen, dlen, B = case
    if noise == "estimated" and plen < 2:
        noise = "scalar"
    lay, fr = _frames(case)
    df = torch.from_numpy(fr).cuda()
    nv = _nv_arg(noise, B, np.random.default_rng(S))
    dn = torch.from_numpy(nv).cuda() if isinstance(nv, np.ndarray) else nv
    for mode in ("linear", "mean"):
        hf = torch.empty((B, S), dtype=torch.complex64, device="cuda")
        z, nvs = D.estimate_csi_device(df, lay, dn, mode=mode, h_out=hf)
        est = torch.empty(B, dtype=torch.float64, device="cuda") if dn is None else None
        y, h = D.strip_pilots_device(df, lay, mode=mode, nv_rows_out=est)
        assert torch.equal(y, df[:, torch.from_numpy(lay.data_positions(S)).cuda()])
        z2, nvs2 = D.equalize_device(y, h, est if dn is None else dn, coh=1)
        assert _teq(h, hf) and _teq(z, z2) and _teq(nvs, nvs2)


# ---- the pipeline against the reference chain ---------------------------------------------------
_CODECS = {}


def _codec(n, rate, **kw):
    key = (n, rate, tuple(sorted(kw.items())))
    if key not in _CODECS:
        _CODECS[key] = M.DVBRCS2_Turbo(n, rate, interleaver="valid-perm", **kw)
    return _CODECS[key]


@pytest.fixture(scope="module")
def chain_ref():
    """Per (rate, mod): 67 framed N = 48 bursts over Rayleigh coh = S with cfo = 1e-4 at 6 dB,
    plen = 2, dlen = 12, and the reference chain's decoder-sign LLRs (restated estimator with
    the pilots' own noise estimate -> restated equaliser -> oracle.demap per symbol)."""
    out = {}
    lay = D.PilotLayout(2, 12)
    for rate, mod in (("1/3", "QPSK"), ("1/2", "16QAM")):
        c = _codec(48, rate)
        bps = D.MODULATIONS[mod]["bps"]
        S = -(-c.n_coded // bps)
        _, frames, n0, _ = W.make_symbols(c, 67, mod, 6.0, 77, "cuda", want_info=False, fading={"K": 0.0, "coh": S},
                                          pilots=lay, cfo=1e-4)
        r = P.estimate(frames.cpu().numpy(), lay.pilots(S), S, 2, 12, nv=None)
        cons = D.constellation(mod)
        _, div_f32, _ = D.demap_mode(np.complex64, cons.dtype, np.float64(1.0))
        llr = -F.demap_per_symbol(r["z"], cons, bps, r["nv_sym"], div_f32)
        out[(rate, mod)] = (lay, frames, n0, llr[:, :c.n_coded].astype(np.float32))
    return out


@pytest.mark.parametrize("rate,mod", [("1/3", "QPSK"), ("1/2", "16QAM")])
def test_run_frames_equals_the_reference_chain(chain_ref, rate, mod):
    c = _codec(48, rate)
    lay, frames, n0, llr = chain_ref[(rate, mod)]
    t, _ = O.trellis()
    want = O.decode_batch(llr, c.N, c.punct["period"], T.puncture_matrix(c.punct), c.iterations, c.perm, c.inv_perm, t)
    dev = torch.device("cuda", 0)
    pipe = W.DevicePipeline(c, mod, 67, dev, csi=True)
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        bits = pipe.run_frames(frames, lay, stream=st).clone()
    st.synchronize()
    assert np.array_equal(bits.cpu().numpy(), want)
    assert 0 < int((bits.cpu().numpy() != 0).sum())
    with pytest.raises(ValueError, match="fused"):
        W.DevicePipeline(c, mod, 67, dev, fused=True, csi=True).run_frames(frames, lay)
    with pytest.raises(ValueError, match="csi=True"):
        W.DevicePipeline(c, mod, 67, dev).run_frames(frames, lay)


def test_run_frames_early_stop_counts(chain_ref):
    c = _codec(48, "1/3", early_stop=True)
    lay, frames, n0, llr = chain_ref[("1/3", "QPSK")]
    t, _ = O.trellis()
    want_bits, _, want_iters = ES.decode_early_stop_batch(llr, c.N, c.punct, c.iterations, c.perm, c.inv_perm, t)
    pipe = W.DevicePipeline(c, "QPSK", 67, torch.device("cuda", 0), csi=True)
    bits = pipe.run_frames(frames, lay)
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    assert np.array_equal(pipe.n_iter[:67].cpu().numpy(), want_iters)


# ---- the generator ------------------------------------------------------------------------------
GEN = dict(mod="16QAM", seed=4242, fading={"K": 4.0, "coh": 5})


def _gen(c, B, lay, cw0=0, ebn0=6.0, cfo=0.0):
    return W.make_symbols(c, B, GEN["mod"], ebn0, GEN["seed"], "cuda", cw0=cw0, want_info=False, fading=GEN["fading"],
                          pilots=lay, cfo=cfo)


@pytest.mark.parametrize("cfo", [0.0, 1e-3])
def test_generator_split_invariance(cfo):
    c, lay = _codec(48, "1/3"), D.PilotLayout(3, 16)
    _, full, _, ht = _gen(c, 1000, lay, cfo=cfo)
    S = 72
    assert tuple(full.shape) == (1000, lay.frame_len(S)) == tuple(ht.shape) and ht.dtype == torch.complex64
    a, b = _gen(c, 400, lay, cfo=cfo), _gen(c, 600, lay, cw0=400, cfo=cfo)
    assert torch.equal(torch.cat([a[1], b[1]]), full) and torch.equal(torch.cat([a[3], b[3]]), ht)


def test_generator_frames_the_fading_symbols():
    c, lay = _codec(48, "1/3"), D.PilotLayout(3, 16)
    S, coh, B = 72, 5, 130
    dpos, ppos = torch.from_numpy(lay.data_positions(S)).cuda(), lay.pilot_positions(S)
    _, frames, n0, ht = _gen(c, B, lay)
    _, syms, n00, gains = W.make_symbols(c, B, GEN["mod"], 6.0, GEN["seed"], "cuda", want_info=False, fading=GEN["fading"])
    assert n0 == n00 and torch.equal(frames[:, dpos], syms)
    g = gains.cpu().numpy()
    assert np.array_equal(ht.cpu().numpy()[:, lay.data_positions(S)], g[:, np.arange(S) // coh])
    blk_gain = g[:, np.minimum(np.arange(lay.n_blocks(S)) * lay.dlen, S - 1) // coh]      # [B, J + 1]
    assert np.array_equal(ht.cpu().numpy()[:, ppos], np.repeat(blk_gain, lay.plen, axis=1))
    # sigma = 0: the pilots are h p rounded to float32
    _, clean, n0c, _ = _gen(c, B, lay, ebn0=float("inf"))
    assert n0c == 0.0
    hp = np.repeat(blk_gain, lay.plen, axis=1).astype(np.complex128) * lay.pilots(S).astype(np.complex128)[None, :]
    assert _eq(clean.cpu().numpy()[:, ppos], hp.astype(np.complex64))
    # the pilots' noise: its own stream, the data's variance
    pn = frames.cpu().numpy()[:, ppos].astype(np.complex128) - hp
    var = np.mean(np.abs(pn) ** 2)
    print("pilot noise variance / N0", var / n0, "over", pn.size)
    assert abs(var / n0 - 1) < 6 / np.sqrt(pn.size)


def test_generator_rotation_is_within_one_ulp_of_its_restatement():
    c, lay = _codec(48, "1/3"), D.PilotLayout(3, 16)
    B, cfo = 130, 1e-3
    _, f0, _, h0 = _gen(c, B, lay, cw0=7)
    _, f1, _, h1 = _gen(c, B, lay, cw0=7, cfo=cfo)
    fg = P.cfo_of(np.arange(7, 7 + B), GEN["seed"], cfo)
    assert np.all(np.abs(fg) < cfo) and fg.min() < -0.5 * cfo and fg.max() > 0.5 * cfo
    for got, base in ((f1, f0), (h1, h0)):
        ref = P.rotate(base.cpu().numpy(), fg).view(np.float32)
        g = got.cpu().numpy().view(np.float32)
        ulp = np.spacing(np.maximum(np.abs(ref), np.abs(g)))
        worst = np.max(np.abs(g.astype(np.float64) - ref) / ulp)
        print("max |device - restatement| in ulp", worst)
        assert worst <= 1.0
    assert not torch.equal(f0, f1)


# ---- statistics ---------------------------------------------------------------------------------
def test_estimator_statistics():
    """N = 48 r = 1/3 QPSK, 256 bursts, plen = 4, dlen = 18, Rayleigh coh = S, no rotation,
    6 dB, one seed.  These bursts are S = 144 symbols, so 9 pilot blocks each (S = 72 and 5
    blocks would be 16QAM).  E|hp - h|^2 = N0 / (plen mean|p|^2): 256 x 9 = 2304 blocks,
    relative standard error 1 / sqrt(2304) = 2.1 %, bound 15 %.  E nv = N0: 2304 x 3 = 6912
    complex degrees of freedom, standard error 1.2 %, bound 10 %."""
    c, lay = _codec(48, "1/3"), D.PilotLayout(4, 18)
    S = -(-c.n_coded // 2)
    assert S == 144 and lay.n_blocks(S) == 9
    _, frames, n0, ht = W.make_symbols(c, 256, "QPSK", 6.0, 31337, "cuda", want_info=False,
                                       fading={"K": 0.0, "coh": S}, pilots=lay, cfo=0.0)
    p = lay.pilots(S)
    hp = P.block_gains(frames.cpu().numpy(), p, S, 4, 18)
    h = ht.cpu().numpy()[:, :1].astype(np.complex128)
    mse = np.mean(np.abs(hp - h) ** 2)
    want = n0 / (4 * np.mean(np.abs(p) ** 2))
    est = torch.empty(256, dtype=torch.float64, device="cuda")
    D.estimate_csi_device(frames, lay, None, floor=0.0, nv_rows_out=est)
    nv = float(est.mean())
    print("block gain mse / expected", mse / want, " mean nv / N0", nv / n0)
    assert abs(mse / want - 1) <= 0.15
    assert abs(nv / n0 - 1) <= 0.10


# ---- ABI argument errors --------------------------------------------------------------------------
def test_abi_refusals_write_nothing():
    L, EINVAL = N.lib(), N.TDEC_EINVAL
    lay = D.PilotLayout(2, 7)
    B, S = 3, 8
    Tn = lay.frame_len(S)
    p = N.ptr
    fr = torch.ones((B, Tn), dtype=torch.complex64, device="cuda")
    pil = lay.pilots_device(S, fr.device)
    z = torch.full((B, S), np.nan, dtype=torch.complex64, device="cuda")
    h = torch.full((B, S), np.nan, dtype=torch.complex64, device="cuda")
    nvs = torch.full((B, S), np.nan, dtype=torch.float64, device="cuda")
    nvo = torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
    nvi = torch.full((B,), 0.1, dtype=torch.float64, device="cuda")
    err = lambda: L.tdec_last_error().decode()  # noqa: E731
    f = L.tdec_csi_pilots_dev
    good = dict(fr=p(fr), B=B, S=S, plen=2, dlen=7, pil=p(pil), mode=0, nv=0.1, nvi=None, z=p(z), nvs=p(nvs), h=p(h),
                nvo=p(nvo))

    def call(**kw):
        a = {**good, **kw}
        return f(0, a["fr"], a["B"], a["S"], a["plen"], a["dlen"], a["pil"], a["mode"], a["nv"], a["nvi"], 0.02,
                 a["z"], a["nvs"], a["h"], a["nvo"], None)
    for k in ("fr", "pil", "z", "nvs"):
        assert call(**{k: None}) == EINVAL and "null pointer" in err()
    for k in ("B", "S", "plen", "dlen"):
        for v in (0, -1):
            assert call(**{k: v}) == EINVAL and ">= 1" in err()
    for m in (2, -1):
        assert call(mode=m) == EINVAL and "mode" in err()
    one = D.PilotLayout(1, 7)
    fr1 = torch.ones((B, one.frame_len(S)), dtype=torch.complex64, device="cuda")
    assert call(fr=p(fr1), plen=1) == EINVAL and "plen >= 2" in err()                        # nv_out with plen == 1
    assert call(fr=p(fr1), plen=1, nvo=None, nv=-1.0) == EINVAL and "no noise source" in err()
    assert call(S=4096, dlen=1) == N.TDEC_EUNSUPPORTED and "2048" in err()
    g = L.tdec_csi_strip_dev
    assert g(0, None, B, S, 2, 7, p(pil), 0, 0.02, p(z), p(h), None, None) == EINVAL and "null pointer" in err()
    assert g(0, p(fr), B, S, 2, 7, p(pil), 0, 0.02, p(z), None, None, None) == EINVAL and "null pointer" in err()
    assert g(0, p(fr), 0, S, 2, 7, p(pil), 0, 0.02, p(z), p(h), None, None) == EINVAL and ">= 1" in err()
    assert g(0, p(fr), B, S, 2, 7, p(pil), 7, 0.02, p(z), p(h), None, None) == EINVAL and "mode" in err()
    assert g(0, p(fr1), B, S, 1, 7, p(pil), 0, 0.02, p(z), p(h), p(nvo), None) == EINVAL and "plen >= 2" in err()
    w = L.tdec_workload_frame_dev
    y = torch.ones((B, S), dtype=torch.complex64, device="cuda")
    out = torch.full((B, Tn), np.nan, dtype=torch.complex64, device="cuda")
    wgood = [0, p(y), p(y), B, S, 1, 2, 7, p(pil), 0.1, 0, 1, 0.0, p(out), None, None]
    for i, v in ((1, None), (2, None), (8, None), (13, None), (3, -1), (4, 0), (5, 0), (6, 0), (7, 0), (9, -0.1),
                 (9, np.nan), (10, -1), (12, -1e-4), (12, np.inf), (12, np.nan)):
        a = list(wgood)
        a[i] = v
        assert w(*a) == EINVAL and "frame arguments" in err(), (i, v)
    a = list(wgood)
    a[3] = 0
    assert w(*a) == 0                                                                        # B = 0: a no-op
    torch.cuda.synchronize()
    for t in (z, h, nvs, nvo, out):
        assert bool(torch.isnan(t.real if t.is_complex() else t).all())
    # and the good call, scalar then [B] noise, does write
    assert call() == 0 and call(nv=-1.0, nvi=p(nvi)) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(z.real).any()) and not bool(torch.isnan(nvo).any())


# ---- ABI argument errors of the framing generator (tests/generator_abi.py) ----
@pytest.mark.parametrize("call,case", GA.params("tdec_workload_frame_dev"))
def test_generator_abi_refusals(call, case):
    GA.check(call, case)
