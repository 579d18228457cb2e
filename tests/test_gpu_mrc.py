"""Receive diversity on the device: the maximal-ratio combiner
against its numpy restatement (tests/mrc_ref.py), the branch generator, and the chain
combine -> demap -> decode against the reference chain.

Every comparison of the combiner is IEEE == with NaN at the same positions and the same
zeros' signs.  The shapes (B, R, S, coh) are the smallest that can go wrong: one symbol;
S odd with coh not dividing it (the 8-byte path); more rows than a wave with S even (the
16-byte path) and per-symbol gains; the most branches with one gain per burst; the
longest row."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import early_stop_ref as ES  # noqa: E402
import fading_ref as F  # noqa: E402
import generator_abi as GA  # noqa: E402
import mrc_ref as MR  # noqa: E402
import pilot_csi_ref as P  # noqa: E402
from oracle import oracle as O  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

SHAPES = [(1, 1, 1, 1), (3, 2, 7, 3), (65, 3, 72, 1), (4, 8, 289, 289), (2, 4, 4512, 47)]
NOISE = ["scalar", "rows", "branches"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _eq(a, b):
    """IEEE ==, NaN at the same positions, and the same zeros' signs."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype in (np.float32, np.complex64) else np.uint64
    na, nb = np.isnan(a.view(a.real.dtype)), np.isnan(b.view(b.real.dtype))
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


def _cn(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)


def _data(B, R, S, coh, seed=0):
    """y [B, R, S] and h [B, R, nh] over many decades, with zero, denormal, huge and non-finite
    gains and non-finite, zero and negative-zero symbols sprinkled in."""
    rng = np.random.default_rng(B * S + R + coh + seed)
    nh = -(-S // coh)
    y = (_cn(rng, B, R, S) * np.float32(10) ** rng.integers(-3, 4, (B, R, S))).astype(np.complex64)
    h = (_cn(rng, B, R, nh) * np.float32(10) ** rng.integers(-2, 3, (B, R, nh))).astype(np.complex64)
    sh = np.array([0, 1e-42 + 3e-43j, np.nan + 1j, 1 + np.inf * 1j, -np.inf, 1e25 - 1e25j, 1e-30j], np.complex64)
    sy = np.array([np.nan, np.inf + 1j, 1 - np.inf * 1j, 0, 1e38 + 1e38j, 1e-44, complex(-0.0, -0.0)], np.complex64)
    hf, yf = h.reshape(-1), y.reshape(-1)
    if hf.size > 1:
        hi = rng.permutation(hf.size)[:len(sh)]
        hf[hi] = sh[:len(hi)]
    if yf.size > 1:
        yi = rng.permutation(yf.size)[:len(sy)]
        yf[yi] = sy[:len(yi)]
    return rng, y, h


def _nv(kind, B, R, rng):
    if kind == "scalar":
        return 0.0371
    return 10.0 ** rng.uniform(-3, 1, B if kind == "rows" else (B, R))


def _dev(nv):
    return torch.from_numpy(nv).cuda() if isinstance(nv, np.ndarray) else nv


def _rows(nv, sl):
    return nv[sl] if isinstance(nv, np.ndarray) else nv


# ---- the combiner ---------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("B,R,S,coh", SHAPES, ids=lambda v: str(v))
def test_kernel_equals_its_numpy_restatement(B, R, S, coh, noise):
    rng, y, h = _data(B, R, S, coh)
    nv = _nv(noise, B, R, rng)
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    z, nvs = D.combine_device(dy, dh, _dev(nv), coh=coh)
    assert z.dtype == torch.complex64 and tuple(z.shape) == (B, S)
    assert nvs.dtype == torch.float64 and tuple(nvs.shape) == (B, S)
    rz, rnv = MR.combine(y, h, nv, coh)
    assert _eq(z.cpu().numpy(), rz) and _eq(nvs.cpu().numpy(), rnv)


@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("B,R,S,coh", SHAPES[1:], ids=lambda v: str(v))
def test_views_one_element_into_their_buffers_and_rows_alone(B, R, S, coh, noise):
    """y, z and nv_sym each one element into a buffer: the 16-byte path is refused and the 8-byte
    one runs, on an even S as well; then single bursts (B = 1) against the batch's rows."""
    rng, y, h = _data(B, R, S, coh, seed=1)
    nv = _nv(noise, B, R, rng)
    rz, rnv = MR.combine(y, h, nv, coh)
    dh = torch.from_numpy(h).cuda()
    ybuf = torch.zeros(B * R * S + 1, dtype=torch.complex64, device="cuda")
    ybuf[1:] = torch.from_numpy(y).cuda().reshape(-1)
    zbuf = torch.full((B * S + 1,), np.nan, dtype=torch.complex64, device="cuda")
    nbuf = torch.full((B * S + 1,), np.nan, dtype=torch.float64, device="cuda")
    oz, onv = zbuf[1:].view(B, S), nbuf[1:].view(B, S)
    assert oz.data_ptr() % 16 == 8 and onv.data_ptr() % 16 == 8
    r = D.combine_device(ybuf[1:].view(B, R, S), dh, _dev(nv), coh=coh, out=oz, nv_out=onv)
    assert r[0] is oz and r[1] is onv
    assert _eq(oz.cpu().numpy(), rz) and _eq(onv.cpu().numpy(), rnv)
    assert bool(torch.isnan(zbuf[0].real)) and bool(torch.isnan(nbuf[0]))      # nothing in front of the views
    # an aligned y with a misaligned z alone also takes the 8-byte path
    dy = torch.from_numpy(y).cuda()
    D.combine_device(dy, dh, _dev(nv), coh=coh, out=oz.zero_())
    assert _eq(oz.cpu().numpy(), rz)
    for b in sorted({0, B // 2, B - 1}):
        z1, n1 = D.combine_device(dy[b:b + 1].contiguous(), dh[b:b + 1].contiguous(),
                                  _dev(_rows(nv, slice(b, b + 1))), coh=coh)
        assert _eq(z1.cpu().numpy(), rz[b:b + 1]) and _eq(n1.cpu().numpy(), rnv[b:b + 1])


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("B,S,coh", [(69, 72, 1), (3, 301, 7), (1, 1, 1), (5, 4512, 4512)])
def test_one_branch_equals_the_equaliser(B, S, coh, rows):
    rng, y, h = _data(B, 1, S, coh, seed=2)
    nv = _nv("rows" if rows else "scalar", B, 1, rng)
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    z, nvs = D.combine_device(dy, dh, _dev(nv), coh=coh)
    ez, env = D.equalize_device(dy[:, 0].contiguous(), dh[:, 0].contiguous(), _dev(nv), coh=coh)
    assert _eq(z.cpu().numpy(), ez.cpu().numpy()) and _eq(nvs.cpu().numpy(), env.cpu().numpy())


def test_nonfinite_and_zero_gains():
    rng = np.random.default_rng(5)
    B, S = 6, 10
    y, h = _cn(rng, B, 2, S), _cn(rng, B, 2, S)
    h[0, 1] = 0                                                       # one dead branch of two
    h[1] = 0                                                          # all dead: an erasure
    h[2, 0, 3] = np.inf                                               # an inf gain: that branch is skipped there
    y[3, 1, 4] = np.nan                                               # a NaN symbol stays local
    h[4, 0, 5], h[4, 1, 5] = np.nan, 0                                # a NaN gain and a zero gain: an erasure
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    for nv in (0.2, np.full((B, 2), 0.2)):
        z, nvs = (t.cpu().numpy() for t in D.combine_device(dy, dh, _dev(nv)))
        rz, rnv = MR.combine(y, h, nv)
        assert _eq(z, rz) and _eq(nvs, rnv)
        ez, env = (t.cpu().numpy() for t in D.equalize_device(dy[:, 0].contiguous(), dh[:, 0].contiguous(), 0.2))
        if np.ndim(nv) == 0:
            assert _eq(z[0], ez[0]) and _eq(nvs[0], env[0])           # the live branch's single-branch result
            e1, n1 = (t.cpu().numpy() for t in D.equalize_device(dy[:, 1].contiguous(), dh[:, 1].contiguous(), 0.2))
            assert _eq(z[2, 3], e1[2, 3]) and _eq(nvs[2, 3], n1[2, 3])
        assert not z[1].any() and np.isposinf(nvs[1]).all()
        assert not z[4, 5] and np.isposinf(nvs[4, 5])
        nan = np.isnan(z.real) | np.isnan(z.imag)
        assert nan[3, 4] and nan.sum() == 1 and np.isfinite(nvs[3]).all()
    nvb = np.full((B, 2), 0.2)
    nvb[5, 1] = np.nan                                                # a NaN per-branch noise: NaN, not a skip
    z, nvs = (t.cpu().numpy() for t in D.combine_device(dy, dh, _dev(nvb)))
    assert np.isnan(z[5].real).all() and np.isnan(nvs[5]).all() and np.isfinite(nvs[0]).all()
    assert _eq(z, MR.combine(y, h, nvb)[0]) and _eq(nvs, MR.combine(y, h, nvb)[1])


# ---- the generator ----------------------------------------------------------------------------------
_CODECS = {}


def _codec(n, rate, **kw):
    key = (n, rate, tuple(sorted(kw.items())))
    if key not in _CODECS:
        _CODECS[key] = M.DVBRCS2_Turbo(n, rate, interleaver="valid-perm", **kw)
    return _CODECS[key]


@pytest.mark.parametrize("K,coh,R", [(0.0, 1, 2), (4.0, 5, 8)])
def test_generator_branches(K, coh, R):
    c = _codec(48, "1/3")
    seed, B, mod = 4242, 1000, "16QAM"
    one = {"K": K, "coh": coh}
    fading = {**one, "branches": R}
    info, full, n0, h = W.make_symbols(c, B, mod, 2.0, seed, "cuda", fading=fading)
    S = -(-c.n_coded // 4)
    nh = -(-S // coh)
    assert tuple(full.shape) == (B, R, S) and tuple(h.shape) == (B, R, nh) and h.dtype == torch.complex64
    # branch 0 is the single-branch generator's output, the info bits are the codeword's
    info1, syms1, n01, h1 = W.make_symbols(c, B, mod, 2.0, seed, "cuda", fading=one)
    assert n01 == n0 and torch.equal(info1, info)
    assert torch.equal(full[:, 0], syms1) and torch.equal(h[:, 0], h1)
    # a 400 + 600 split equals one batch of 1000 exactly, gains included
    a = W.make_symbols(c, 400, mod, 2.0, seed, "cuda", cw0=0, want_info=False, fading=fading)
    b = W.make_symbols(c, 600, mod, 2.0, seed, "cuda", cw0=400, want_info=False, fading=fading)
    assert torch.equal(torch.cat([a[1], b[1]]), full) and torch.equal(torch.cat([a[3], b[3]]), h)
    # every branch carries the same codeword: without noise, y_b = h_b x with branch 0's x
    _, clean, _, hc = W.make_symbols(c, 64, mod, 1000.0, seed, "cuda", want_info=False, fading=fading)
    assert torch.equal(hc, h[:64])
    hs = hc.cpu().numpy().astype(np.complex128)[:, :, np.arange(S) // coh]
    x = W.make_symbols(c, 64, mod, 1000.0, seed, "cuda", want_info=False)[1].cpu().numpy().astype(np.complex128)
    err = np.max(np.abs(clean.cpu().numpy() - hs * x[:, None, :]))
    print("max |clean branch - h x|", err)
    assert err < 2e-5
    # the branches' noises differ, and the gains are the restatement's
    noise = full[:64].cpu().numpy().astype(np.complex128) - hs * x[:, None, :]
    assert np.mean(np.abs(noise[:, 1] - noise[:, 0]) ** 2) > n0       # independent: E|n_1 - n_0|^2 = 2 N0
    ref = MR.gains(np.arange(B), R, nh, seed, K)
    print("max |gain - restatement|", np.max(np.abs(h.cpu().numpy() - ref)))
    assert np.max(np.abs(h.cpu().numpy() - ref)) < 2e-5


@pytest.mark.parametrize("cfo", [0.0, 1e-3])
def test_generator_frames_the_branches(cfo):
    c, lay = _codec(48, "1/3"), D.PilotLayout(3, 16)
    mod, seed, R = "16QAM", 4242, 3
    one = {"K": 4.0, "coh": 5}
    fading = {**one, "branches": R}
    S = 72
    gen = lambda B, cw0, f: W.make_symbols(c, B, mod, 6.0, seed, "cuda", cw0=cw0, want_info=False, fading=f,  # noqa: E731
                                           pilots=lay, cfo=cfo)
    _, full, n0, ht = gen(1000, 0, fading)
    assert tuple(full.shape) == (1000, R, lay.frame_len(S)) == tuple(ht.shape)
    _, f1, n01, ht1 = gen(1000, 0, one)
    assert n01 == n0 and torch.equal(full[:, 0], f1) and torch.equal(ht[:, 0], ht1)
    a, b = gen(400, 0, fading), gen(600, 400, fading)
    assert torch.equal(torch.cat([a[1], b[1]]), full) and torch.equal(torch.cat([a[3], b[3]]), ht)
    # the data positions are the unframed branches; the rotation is the codeword's, shared
    if cfo == 0.0:
        _, syms, _, gains = W.make_symbols(c, 1000, mod, 6.0, seed, "cuda", want_info=False, fading=fading)
        dpos = torch.from_numpy(lay.data_positions(S)).cuda()
        assert torch.equal(full[:, :, dpos], syms)
        ppos = lay.pilot_positions(S)
        pil = full.cpu().numpy()[:, :, ppos]
        assert not np.array_equal(pil[:, 1], pil[:, 0]) and not np.array_equal(pil[:, 2], pil[:, 1])
    else:
        h0 = ht[:130].cpu().numpy().astype(np.complex128)
        _, _, _, hu = W.make_symbols(c, 130, mod, 6.0, seed, "cuda", want_info=False, fading=fading, pilots=lay)
        rot = h0 / hu.cpu().numpy().astype(np.complex128)             # exp(j 2 pi f_g t) per position
        assert np.max(np.abs(rot[:, 1] - rot[:, 0])) < 1e-5 and np.max(np.abs(rot[:, 2] - rot[:, 0])) < 1e-5
        assert np.max(np.abs(rot[:, 0, -1] - 1)) > 1e-3


def test_branch_statistics():
    """N = 48 r = 1/3 QPSK, 256 bursts, R = 2, Rayleigh, coh = 1: n = 256 S gains per branch.
    sum_r |h_r|^2 has mean 2 and variance 2 (two unit exponentials), so its mean's relative
    standard error is 1 / sqrt(2 n), under 1 %: bound 3 %.  h_0 conj(h_1) of independent unit
    gains has mean 0 and E|.|^2 = 1: |mean| <= 6 / sqrt(n)."""
    c = _codec(48, "1/3")
    _, _, _, h = W.make_symbols(c, 256, "QPSK", 6.0, 31337, "cuda", want_info=False,
                                fading={"K": 0.0, "coh": 1, "branches": 2})
    g = h.cpu().numpy().astype(np.complex128)
    n = 256 * g.shape[2]
    assert g.shape == (256, 2, 144) and 1 / np.sqrt(2 * n) < 0.01
    power = float(np.mean(np.sum(np.abs(g) ** 2, axis=1)))
    cross = abs(np.mean(g[:, 0] * np.conj(g[:, 1])))
    print("mean sum |h_r|^2", power, " |mean h_0 conj(h_1)|", cross, "bound", 6 / np.sqrt(n))
    assert abs(power / 2 - 1) <= 0.03
    assert cross <= 6 / np.sqrt(n)


# ---- combine -> demap -> decode against the reference chain ---------------------------------------
PAIRS = [("1/3", "QPSK"), ("1/2", "16QAM")]
LAY = (2, 12)
NB = 67


def _llr(z, nvs, mod, c):
    cons = D.constellation(mod)
    _, div_f32, _ = D.demap_mode(np.complex64, cons.dtype, np.float64(1.0))
    llr = -F.demap_per_symbol(z, cons, D.MODULATIONS[mod]["bps"], nvs, div_f32)     # decoder sign
    return llr[:, :c.n_coded].astype(np.float32)


@pytest.fixture(scope="module")
def chain_ref():
    """Per (rate, mod): 67 N = 48 bursts on R = 2 branches over Rayleigh coh = S at 4 dB, unframed
    with their gains and framed (plen = 2, dlen = 12, cfo = 1e-4), and the reference chain's
    decoder-sign LLRs for both: restated combiner (behind the restated pilot estimator's strip
    for the frames) -> oracle.demap per symbol.  Computed once."""
    out = {}
    lay = D.PilotLayout(*LAY)
    for rate, mod in PAIRS:
        c = _codec(48, rate)
        S = -(-c.n_coded // D.MODULATIONS[mod]["bps"])
        fading = {"K": 0.0, "coh": S, "branches": 2}
        _, syms, n0, h = W.make_symbols(c, NB, mod, 4.0, 77, "cuda", want_info=False, fading=fading)
        _, frames, n0f, _ = W.make_symbols(c, NB, mod, 4.0, 77, "cuda", want_info=False, fading=fading, pilots=lay,
                                           cfo=1e-4)
        assert n0f == n0
        z, nvs = MR.combine(syms.cpu().numpy(), h.cpu().numpy(), n0, S)
        r = P.estimate(frames.cpu().numpy().reshape(NB * 2, -1), lay.pilots(S), S, *LAY, nv=n0)
        ys, hs = r["y"].reshape(NB, 2, S), r["h"].reshape(NB, 2, S)
        zf, nvf = MR.combine(ys, hs, n0, 1)
        out[(rate, mod)] = dict(lay=lay, syms=syms, h=h, n0=n0, frames=frames, S=S, llr=_llr(z, nvs, mod, c),
                                llr_frames=_llr(zf, nvf, mod, c), ys=ys, hs=hs, est=r["nv"].reshape(NB, 2))
    return out


def _oracle(c, llr):
    t, _ = O.trellis()
    return O.decode_batch(llr, c.N, c.punct["period"], T.puncture_matrix(c.punct), c.iterations, c.perm, c.inv_perm, t,
                          want_lfinal=True)


def _lfinal(c, pipe, n):
    """L_final of the planes the pipeline's last batch demapped."""
    bits = torch.empty((n, c.k_info), dtype=torch.int32, device="cuda")
    lf = torch.empty((n, c.k_info), dtype=torch.float64, device="cuda")
    c.decode_planes_device(pipe.planes, n, bits, lfinal=lf)
    return bits.cpu().numpy(), lf.cpu().numpy()


@pytest.mark.parametrize("rate,mod", PAIRS)
def test_run_and_run_frames_equal_the_reference_chain(chain_ref, rate, mod):
    c = _codec(48, rate)
    k = chain_ref[(rate, mod)]
    dev = torch.device("cuda", 0)
    pipe = W.DevicePipeline(c, mod, NB, dev, csi=True)
    # run() with [B, R, S] symbols and their gains, on a stream of its own
    want, want_lf = _oracle(c, k["llr"])
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        bits = pipe.run(k["syms"], k["n0"], stream=st, csi=k["h"], coh=k["S"]).clone()
    st.synchronize()
    assert np.array_equal(bits.cpu().numpy(), want) and 0 < int((want != 0).sum())
    b2, lf = _lfinal(c, pipe, NB)
    assert np.array_equal(b2, want) and np.array_equal(lf, want_lf)
    nv_rows = torch.full((NB,), float(k["n0"]), dtype=torch.float64, device=dev)
    assert torch.equal(pipe.run(k["syms"], nv_rows, csi=k["h"], coh=k["S"]), bits)
    # run_frames() with [B, R, T] frames and the known noise variance: strip, then the common form
    want, want_lf = _oracle(c, k["llr_frames"])
    bits = pipe.run_frames(k["frames"], k["lay"], k["n0"]).clone()
    assert np.array_equal(bits.cpu().numpy(), want)
    b2, lf = _lfinal(c, pipe, NB)
    assert np.array_equal(b2, want) and np.array_equal(lf, want_lf)
    # refusals
    with pytest.raises(ValueError, match="fused"):
        W.DevicePipeline(c, mod, NB, dev, fused=True, csi=True).run_frames(k["frames"], k["lay"])
    with pytest.raises(ValueError, match="fused"):
        W.DevicePipeline(c, mod, NB, dev, fused=True, csi=True).run(k["syms"], k["n0"], csi=k["h"], coh=k["S"])
    with pytest.raises(ValueError, match="csi=True"):
        W.DevicePipeline(c, mod, NB, dev).run_frames(k["frames"], k["lay"])
    with pytest.raises(ValueError, match="gains"):
        pipe.run(k["syms"], k["n0"])


@pytest.mark.parametrize("rate,mod", PAIRS)
def test_run_frames_with_estimated_noise_is_strip_then_per_branch_combine(chain_ref, rate, mod):
    c = _codec(48, rate)
    k = chain_ref[(rate, mod)]
    S, lay = k["S"], k["lay"]
    pipe = W.DevicePipeline(c, mod, NB, torch.device("cuda", 0), csi=True)
    bits = pipe.run_frames(k["frames"], lay).clone()
    z, nvs = pipe.z[:NB].clone(), pipe.nv_sym[:NB].clone()
    est = torch.empty(NB * 2, dtype=torch.float64, device="cuda")
    y, h = D.strip_pilots_device(k["frames"].view(NB * 2, -1), lay, nv_rows_out=est)
    assert _eq(y.cpu().numpy().reshape(NB, 2, S), k["ys"]) and _eq(h.cpu().numpy().reshape(NB, 2, S), k["hs"])
    assert _eq(est.cpu().numpy().reshape(NB, 2), k["est"])
    cz, cnv = D.combine_device(y.view(NB, 2, S), h.view(NB, 2, S), est.view(NB, 2))
    assert torch.equal(z.view(torch.int32), cz.view(torch.int32)) and torch.equal(nvs.view(torch.int64), cnv.view(torch.int64))
    rz, rnv = MR.combine(k["ys"], k["hs"], k["est"], 1)
    assert _eq(z.cpu().numpy(), rz) and _eq(nvs.cpu().numpy(), rnv)
    # and the same bits as the two-launch demap + decode on those arrays
    planes = torch.empty_like(pipe.planes)
    cons = D.constellation(mod)
    div32 = D.demap_mode(np.complex64, cons.dtype, np.float64(1.0))[1]
    c.demap_planes_device(cz, cons, D.MODULATIONS[mod]["bps"], cnv, planes, div_f32=div32)
    b2 = torch.empty_like(bits)
    c.decode_planes_device(planes, NB, b2)
    assert torch.equal(bits, b2)


def test_early_stop_counts(chain_ref):
    c = _codec(48, "1/3", early_stop=True, es_decoder="tile")
    k = chain_ref[("1/3", "QPSK")]
    t, _ = O.trellis()
    want_bits, _, want_iters = ES.decode_early_stop_batch(k["llr"], c.N, c.punct, c.iterations, c.perm, c.inv_perm, t)
    pipe = W.DevicePipeline(c, "QPSK", NB, torch.device("cuda", 0), csi=True)
    bits = pipe.run(k["syms"], k["n0"], csi=k["h"], coh=k["S"])
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    assert np.array_equal(pipe.n_iter[:NB].cpu().numpy(), want_iters)
    assert want_iters.min() < c.iterations


def test_two_dimensional_inputs_are_unchanged(chain_ref):
    """run, run_frames and make_symbols without the new arguments: the same calls they made
    before, compared with those calls made here directly, and with the one-branch 3-D forms."""
    rate, mod = PAIRS[1]
    c = _codec(48, rate)
    k = chain_ref[(rate, mod)]
    S, lay, n0 = k["S"], k["lay"], k["n0"]
    cons, bps = D.constellation(mod), D.MODULATIONS[mod]["bps"]
    div32 = D.demap_mode(np.complex64, cons.dtype, np.float64(1.0))[1]
    one = {"K": 0.0, "coh": S}
    # make_symbols: the single-branch entry points called directly
    info, syms, n01, h = W.make_symbols(c, NB, mod, 4.0, 77, "cuda", fading=one)
    _, frames, _, ht = W.make_symbols(c, NB, mod, 4.0, 77, "cuda", want_info=False, fading=one, pilots=lay, cfo=1e-4)
    assert n01 == n0 and syms.dim() == 2 and frames.dim() == 2
    table = np.ascontiguousarray(cons.astype(np.complex64)).view(np.float32)
    s2, h2, i2 = torch.empty_like(syms), torch.empty_like(h), torch.empty_like(info)
    sigma = float(np.sqrt(n0 / 2))
    c.handle.call("tdec_workload_fading_dev", NB, 0, 77, N.ptr(table), len(cons), bps, sigma, 0.0, S, N.ptr(s2), N.ptr(h2),
                  N.ptr(i2), None)
    f2, t2 = torch.empty_like(frames), torch.empty_like(ht)
    N.check(N.lib().tdec_workload_frame_dev(0, N.ptr(s2), N.ptr(h2), NB, S, S, lay.plen, lay.dlen,
                                            N.ptr(lay.pilots_device(S, f2.device)), sigma, 0, 77, 1e-4, N.ptr(f2), N.ptr(t2),
                                            None))
    torch.cuda.synchronize()
    assert torch.equal(s2, syms) and torch.equal(h2, h) and torch.equal(i2, info)
    assert torch.equal(f2, frames) and torch.equal(t2, ht)
    assert torch.equal(syms, k["syms"][:, 0]) and torch.equal(frames, k["frames"][:, 0])

    def decode(z, nvs):
        planes = torch.empty(c.planes_bytes(NB) // 4, dtype=torch.float32, device="cuda")
        c.demap_planes_device(z, cons, bps, nvs, planes, div_f32=div32)
        bits = torch.empty((NB, c.k_info), dtype=torch.int32, device="cuda")
        c.decode_planes_device(planes, NB, bits)
        return bits
    pipe = W.DevicePipeline(c, mod, NB, torch.device("cuda", 0), csi=True)
    # run(): equalize_device -> demap -> decode
    bits = pipe.run(syms, n0, csi=h, coh=S).clone()
    assert torch.equal(bits, decode(*D.equalize_device(syms, h, n0, coh=S)))
    assert torch.equal(pipe.run(syms[:, None].contiguous(), n0, csi=h[:, None].contiguous(), coh=S), bits)
    # run_frames(): estimate_csi_device -> demap -> decode, known and estimated noise
    for nv in (n0, None):
        bits = pipe.run_frames(frames, lay, nv).clone()
        assert torch.equal(bits, decode(*D.estimate_csi_device(frames, lay, nv)))
    bits = pipe.run_frames(frames, lay, n0).clone()
    assert torch.equal(pipe.run_frames(frames[:, None].contiguous(), lay, n0), bits)


# ---- ABI argument errors ------------------------------------------------------------------------------
def test_abi_refusals_write_nothing():
    L, EINVAL = N.lib(), N.TDEC_EINVAL
    B, R, S = 3, 2, 8
    p = N.ptr
    y = torch.ones((B, R, S), dtype=torch.complex64, device="cuda")
    z = torch.full((B, S), np.nan, dtype=torch.complex64, device="cuda")
    nvs = torch.full((B, S), np.nan, dtype=torch.float64, device="cuda")
    nvr = torch.full((B,), 0.1, dtype=torch.float64, device="cuda")
    nvb = torch.full((B, R), 0.1, dtype=torch.float64, device="cuda")
    good = dict(y=p(y), h=p(y), B=B, R=R, S=S, coh=1, nv=0.1, rows=None, br=None, z=p(z), nvs=p(nvs))

    def call(**kw):
        a = {**good, **kw}
        return L.tdec_combine_dev(0, a["y"], a["h"], a["B"], a["R"], a["S"], a["coh"], a["nv"], a["rows"], a["br"], a["z"],
                                  a["nvs"], None)
    for kw in (dict(y=None), dict(h=None), dict(z=None), dict(nvs=None), dict(B=-1), dict(S=-1), dict(coh=0), dict(coh=-3),
               dict(R=0), dict(R=9), dict(R=-1), dict(rows=p(nvr), br=p(nvb)), dict(R=9, B=0), dict(coh=0, S=0)):
        assert call(**kw) == EINVAL and "combine" in L.tdec_last_error().decode(), kw
    assert call(B=0, y=None, h=None, z=None, nvs=None) == 0
    assert call(S=0, y=None, h=None, z=None, nvs=None) == 0
    # the generators
    c = _codec(48, "1/3")
    tab = np.ascontiguousarray(D.constellation("16QAM").astype(np.complex64)).view(np.float32)
    Sw = -(-c.handle.enc_len // 4)
    sy = torch.full((B, R, Sw), np.nan, dtype=torch.complex64, device="cuda")
    sh = torch.full((B, R, Sw), np.nan, dtype=torch.complex64, device="cuda")
    wb = L.tdec_workload_branches_dev
    for r_, k_, coh, gains in ((0, 0.0, 1, sh), (9, 0.0, 1, sh), (R, -1.0, 1, sh), (R, np.nan, 1, sh), (R, 0.0, 0, sh),
                               (R, 0.0, 1, None)):
        assert wb(c.handle.h, B, r_, 0, 1, p(tab), 16, 4, 0.1, k_, coh, p(sy), p(gains), None, None) == EINVAL
    assert wb(c.handle.h, 0, R, 0, 1, p(tab), 16, 4, 0.1, 0.0, 1, None, None, None, None) == 0
    lay = D.PilotLayout(2, 7)
    pil = lay.pilots_device(S, y.device)
    out = torch.full((B, R, lay.frame_len(S)), np.nan, dtype=torch.complex64, device="cuda")
    wf = L.tdec_workload_frame_branches_dev
    wgood = [0, p(y), p(y), B, R, S, 1, 2, 7, p(pil), 0.1, 0, 1, 0.0, p(out), None, None]
    for i, v in ((1, None), (2, None), (9, None), (14, None), (3, -1), (4, 0), (4, 9), (5, 0), (6, 0), (7, 0), (8, 0),
                 (10, -0.1), (11, -1), (13, -1e-4), (13, np.inf)):
        a = list(wgood)
        a[i] = v
        assert wf(*a) == EINVAL and "frame arguments" in L.tdec_last_error().decode(), (i, v)
    a = list(wgood)
    a[3] = 0
    assert wf(*a) == 0
    torch.cuda.synchronize()
    for t in (z, sy, sh, out):
        assert bool(torch.isnan(t.real).all())
    assert bool(torch.isnan(nvs).all())
    for bad in ({"K": 0.0, "coh": 1, "branches": 0}, {"K": 0.0, "coh": 1, "branches": 9}, {"K": 0.0, "branches": 2, "x": 1}):
        with pytest.raises(ValueError):
            W.make_symbols(c, B, "16QAM", 2.0, 1, "cuda", fading=bad)


# ---- ABI argument errors of the branch generators (tests/generator_abi.py) ----
@pytest.mark.parametrize("call,case", GA.params("tdec_workload_branches_dev", "tdec_workload_frame_branches_dev"))
def test_generator_abi_refusals(call, case):
    GA.check(call, case)


# ---- the generators on a ragged shape -------------------------------------------------------------
@pytest.mark.parametrize("cfo", [0.0, 1e-3])
def test_generators_on_a_ragged_shape(cfo):
    """65 codewords (two tiles, the second ragged) of N = 64 r = 1/2 on 8PSK: 256 coded bits in
    S = 86 symbols, the last one padded (every rate of N = 48 gives a multiple of 3 bits, so the
    next block size stands in); coh = 7 does not divide S; R = 3; plen = 2, dlen = 5.
    One launch of each generator.  Branch 0 is the single-branch calls' output and the frames
    hold the symbols and gains, all bit for bit; the gains are their restatements' to the 2e-5
    of the float32 Box-Muller (as above); the rotation is within one ulp of its restatement;
    and the equaliser, combiner and estimator on these arrays are IEEE == their restatements."""
    c, lay = _codec(64, "1/2"), D.PilotLayout(2, 5)
    B, R, coh, K, mod, seed, cw0 = 65, 3, 7, 2.0, "8PSK", 99, 11
    S, one = -(-c.n_coded // 3), {"K": K, "coh": coh}
    nh = -(-S // coh)
    assert c.n_coded % 3 and S % coh and S % lay.dlen
    gen = lambda f, **kw: W.make_symbols(c, B, mod, 6.0, seed, "cuda", cw0=cw0, fading=f, **kw)  # noqa: E731
    info, syms, n0, h = gen({**one, "branches": R})
    info1, syms1, _, h1 = gen(one)
    _, frames, _, ht = gen({**one, "branches": R}, pilots=lay, cfo=cfo)
    _, frames1, _, ht1 = gen(one, pilots=lay, cfo=cfo)
    T_ = lay.frame_len(S)
    assert tuple(syms.shape) == (B, R, S) and tuple(h.shape) == (B, R, nh) and tuple(frames.shape) == (B, R, T_) == tuple(ht.shape)
    assert torch.equal(info, info1) and torch.equal(syms[:, 0], syms1) and torch.equal(h[:, 0], h1)
    assert torch.equal(frames[:, 0], frames1) and torch.equal(ht[:, 0], ht1)
    assert torch.equal(info, W.info_bits(c, B, seed, "cuda", cw0=cw0))
    g, y = h.cpu().numpy(), syms.cpu().numpy()
    for got, ref in ((g, MR.gains(np.arange(cw0, cw0 + B), R, nh, seed, K)), (g[:, 0], F.gains(np.arange(cw0, cw0 + B), nh, seed, K))):
        print("max |gain - restatement|", np.max(np.abs(got - ref)))
        assert np.max(np.abs(got - ref)) < 2e-5
    dpos, ppos = P.data_positions(S, 2, 5), lay.pilot_positions(S)
    blk = g[:, :, np.minimum(np.arange(lay.n_blocks(S)) * 5, S - 1) // coh]               # [B, R, J + 1]
    if cfo == 0.0:
        f, t = frames.cpu().numpy(), ht.cpu().numpy()
        assert _eq(f[:, :, dpos], y) and _eq(t[:, :, dpos], g[:, :, np.arange(S) // coh])
        assert _eq(t[:, :, ppos], np.repeat(blk, 2, axis=2))
    else:
        _, f0, _, t0 = gen({**one, "branches": R}, pilots=lay)
        fg = np.repeat(P.cfo_of(np.arange(cw0, cw0 + B), seed, cfo), R)
        for got, base in ((frames, f0), (ht, t0)):
            ref = P.rotate(base.cpu().numpy().reshape(B * R, T_), fg).view(np.float32)
            d = got.cpu().numpy().reshape(B * R, T_).view(np.float32)
            worst = np.max(np.abs(d.astype(np.float64) - ref) / np.spacing(np.maximum(np.abs(ref), np.abs(d))))
            print("max |device - restatement| in ulp", worst)
            assert worst <= 1.0
    # the receivers' front ends on these arrays
    z, nvs = D.combine_device(syms, h, n0, coh=coh)
    rz, rnv = MR.combine(y, g, n0, coh)
    assert _eq(z.cpu().numpy(), rz) and _eq(nvs.cpu().numpy(), rnv)
    z, nvs = D.equalize_device(syms1, h1, n0, coh=coh)
    rz, rnv = F.equalize(y[:, 0], g[:, 0], n0, coh)
    assert _eq(z.cpu().numpy(), rz) and _eq(nvs.cpu().numpy(), rnv)
    z, nvs = D.estimate_csi_device(frames1, lay, n0)
    want = P.estimate(frames1.cpu().numpy(), lay.pilots(S), S, 2, 5, "linear", n0)
    assert _eq(z.cpu().numpy(), want["z"]) and _eq(nvs.cpu().numpy(), want["nv_sym"])
