"""Transmit diversity on the device (include/stbc.h): the Alamouti combiner
against its numpy restatement (tests/stbc_ref.py), the generator's 2 x R link, and the chain
combine -> demap -> decode against the reference chain.

Every comparison of the combiner is IEEE == with NaN at the same positions and the same zeros'
signs.  The shapes (B, R, S, coh): one symbol (an odd S: the pad slot); one pair; an odd S over
several rows and branches; more rows than a wave with S even (the 16-byte stores), several blocks
and a block boundary between pairs; the most branches with an odd S and one gain block per burst;
the longest row."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import early_stop_ref as ES  # noqa: E402
import fading_ref as F  # noqa: E402
import generator_cases as GC  # noqa: E402
import llrq_ref as LQ  # noqa: E402
import stbc_ref as SR  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import workload_ref as WR  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

SHAPES = [(1, 1, 1, 2), (2, 1, 2, 2), (3, 2, 7, 2), (65, 3, 72, 4), (4, 8, 289, 290), (2, 4, 4512, 48)]
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
    """y [B, R, S2] and h [B, R, 2, nh] over many decades, with zero, denormal, huge and non-finite
    gains and non-finite, zero and negative-zero slots sprinkled in."""
    rng = np.random.default_rng(B * S + R + coh + seed)
    S2 = SR.s2_of(S)
    nh = -(-S2 // coh)
    y = (_cn(rng, B, R, S2) * np.float32(10) ** rng.integers(-3, 4, (B, R, S2))).astype(np.complex64)
    h = (_cn(rng, B, R, 2, nh) * np.float32(10) ** rng.integers(-2, 3, (B, R, 2, nh))).astype(np.complex64)
    sh = np.array([0, 1e-42 + 3e-43j, np.nan + 1j, 1 + np.inf * 1j, -np.inf, 1e25 - 1e25j, 1e-30j], np.complex64)
    sy = np.array([np.nan, np.inf + 1j, 1 - np.inf * 1j, 0, 1e38 + 1e38j, 1e-44, complex(-0.0, -0.0)], np.complex64)
    hf, yf = h.reshape(-1), y.reshape(-1)
    if hf.size > 2:
        hi = rng.permutation(hf.size)[:len(sh)]
        hf[hi] = sh[:len(hi)]
    if yf.size > 2:
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


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


# ---- the combiner ---------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("B,R,S,coh", SHAPES, ids=lambda v: str(v))
def test_kernel_equals_its_numpy_restatement(B, R, S, coh, noise):
    rng, y, h = _data(B, R, S, coh)
    nv = _nv(noise, B, R, rng)
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    z, nvs = D.stbc_combine_device(dy, dh, _dev(nv), S=S, coh=coh)
    assert z.dtype == torch.complex64 and tuple(z.shape) == (B, S)
    assert nvs.dtype == torch.float64 and tuple(nvs.shape) == (B, S)
    rz, rnv = SR.combine(y, h, nv, S, coh)
    assert _eq(z.cpu().numpy(), rz) and _eq(nvs.cpu().numpy(), rnv)


@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("B,R,S,coh", SHAPES[1:], ids=lambda v: str(v))
def test_views_one_element_into_their_buffers_and_rows_alone(B, R, S, coh, noise):
    """y, z and nv_sym each one element into a buffer: 8-byte loads and stores, on an even S as well, and
    nothing in front of the views or (an odd S: the pad slot's second output) behind them is written; then
    single bursts (B = 1) against the batch's rows."""
    rng, y, h = _data(B, R, S, coh, seed=1)
    nv = _nv(noise, B, R, rng)
    S2 = SR.s2_of(S)
    rz, rnv = SR.combine(y, h, nv, S, coh)
    dh = torch.from_numpy(h).cuda()
    ybuf = torch.zeros(B * R * S2 + 1, dtype=torch.complex64, device="cuda")
    ybuf[1:] = torch.from_numpy(y).cuda().reshape(-1)
    zbuf = torch.full((B * S + 2,), np.nan, dtype=torch.complex64, device="cuda")
    nbuf = torch.full((B * S + 2,), np.nan, dtype=torch.float64, device="cuda")
    oz, onv = zbuf[1:-1].view(B, S), nbuf[1:-1].view(B, S)
    assert oz.data_ptr() % 16 == 8 and onv.data_ptr() % 16 == 8
    r = D.stbc_combine_device(ybuf[1:].view(B, R, S2), dh, _dev(nv), S=S, coh=coh, out=oz, nv_out=onv)
    assert r[0] is oz and r[1] is onv
    assert _eq(oz.cpu().numpy(), rz) and _eq(onv.cpu().numpy(), rnv)
    for guard in (0, -1):
        assert bool(torch.isnan(zbuf[guard].real)) and bool(torch.isnan(nbuf[guard]))
    # an aligned y with a misaligned z alone also takes the 8-byte stores; a misaligned y with aligned outputs the
    # 8-byte loads
    dy = torch.from_numpy(y).cuda()
    D.stbc_combine_device(dy, dh, _dev(nv), S=S, coh=coh, out=oz.zero_())
    assert _eq(oz.cpu().numpy(), rz)
    z2, n2 = D.stbc_combine_device(ybuf[1:].view(B, R, S2), dh, _dev(nv), S=S, coh=coh)
    assert _eq(z2.cpu().numpy(), rz) and _eq(n2.cpu().numpy(), rnv)
    for b in sorted({0, B // 2, B - 1}):
        z1, n1 = D.stbc_combine_device(dy[b:b + 1].contiguous(), dh[b:b + 1].contiguous(),
                                       _dev(_rows(nv, slice(b, b + 1))), S=S, coh=coh)
        assert _eq(z1.cpu().numpy(), rz[b:b + 1]) and _eq(n1.cpu().numpy(), rnv[b:b + 1])


@pytest.mark.parametrize("S", [1, 7, 289])
def test_an_odd_length_leaves_the_element_behind_the_outputs_alone(S):
    """Aligned outputs, odd S: the pad slot's second output would land on the next row's first element, or
    behind the last row."""
    B, R, coh = 3, 2, 2
    rng, y, h = _data(B, R, S, coh, seed=3)
    zbuf = torch.full((B * S + 1,), np.nan, dtype=torch.complex64, device="cuda")
    nbuf = torch.full((B * S + 1,), np.nan, dtype=torch.float64, device="cuda")
    D.stbc_combine_device(torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(), 0.2, S=S, coh=coh,
                          out=zbuf[:-1].view(B, S), nv_out=nbuf[:-1].view(B, S))
    rz, rnv = SR.combine(y, h, 0.2, S, coh)
    assert _eq(zbuf[:-1].cpu().numpy().reshape(B, S), rz) and _eq(nbuf[:-1].cpu().numpy().reshape(B, S), rnv)
    assert bool(torch.isnan(zbuf[-1].real)) and float(zbuf[-1].imag) == 0.0 and bool(torch.isnan(nbuf[-1]))   # NaN + 0j


def test_dead_infinite_and_nan_gains_symbols_and_noise():
    rng = np.random.default_rng(5)
    B, S, coh = 8, 20, 2
    y, h = _cn(rng, B, 2, S), _cn(rng, B, 2, 2, S // coh)
    h[0, 1] = 0                                                       # one dead branch of two (both its paths)
    h[1] = 0                                                          # all dead: an erasure
    h[2, 0, 1, 3] = np.inf                                            # an inf gain on one path: that branch is skipped there
    y[3, 1, 9] = np.nan                                               # a NaN slot stays in its pair
    h[4, 0, 0, 5], h[4, 1] = np.nan, 0                                # a NaN gain and a dead branch: an erasure
    h[6, :, 1] = 0                                                    # antenna 1 dead everywhere: the rows still combine
    h[7, 0, :, 2] = 0                                                 # both antennas of one branch in one block
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    for nv in (0.2, np.full((B, 2), 0.2)):
        z, nvs = _np(*D.stbc_combine_device(dy, dh, _dev(nv), coh=coh))
        rz, rnv = SR.combine(y, h, nv, coh=coh)
        assert _eq(z, rz) and _eq(nvs, rnv)
        if np.ndim(nv) == 0:                                          # the live branch alone
            z0, n0 = _np(*D.stbc_combine_device(dy[:, :1].contiguous(), dh[:, :1].contiguous(), 0.2, coh=coh))
            z1, n1 = _np(*D.stbc_combine_device(dy[:, 1:].contiguous(), dh[:, 1:].contiguous(), 0.2, coh=coh))
            assert _eq(z[0], z0[0]) and _eq(nvs[0], n0[0])
            assert _eq(z[2, 6:8], z1[2, 6:8]) and _eq(nvs[2, 6:8], n1[2, 6:8])
            assert _eq(z[7, 4:6], z1[7, 4:6]) and _eq(nvs[7, 4:6], n1[7, 4:6])
        assert not z[1].any() and np.isposinf(nvs[1]).all()
        assert not z[4, 10:12].any() and np.isposinf(nvs[4, 10:12]).all()
        assert np.isfinite(nvs[6]).all() and np.isfinite(z[6].real).all()
        nan = np.isnan(z.real) | np.isnan(z.imag)
        assert nan[3, 8] and nan[3, 9] and nan.sum() == 2 and np.isfinite(nvs[3]).all()
    nvb = np.full((B, 2), 0.2)
    nvb[5, 1] = np.nan                                                # a NaN per-branch noise: NaN, not a skip
    z, nvs = _np(*D.stbc_combine_device(dy, dh, _dev(nvb), coh=coh))
    assert np.isnan(z[5].real).all() and np.isnan(nvs[5]).all() and np.isfinite(nvs[0]).all()
    rz, rnv = SR.combine(y, h, nvb, coh=coh)
    assert _eq(z, rz) and _eq(nvs, rnv)


@pytest.mark.parametrize("B,R,S,coh", [(69, 1, 72, 2), (3, 1, 301, 14), (5, 3, 144, 144), (2, 8, 7, 4)])
def test_a_silent_second_antenna_is_the_equaliser_or_the_combiner_on_the_even_slots(B, R, S, coh):
    rng = np.random.default_rng(B + S)
    S2 = SR.s2_of(S)
    nh = -(-S2 // coh)
    y = (_cn(rng, B, R, S2) * np.float32(10) ** rng.integers(-3, 4, (B, R, S2))).astype(np.complex64)
    h = np.zeros((B, R, 2, nh), np.complex64)
    h[:, :, 0] = _cn(rng, B, R, nh)
    h[0, 0, 0, 0] = 0
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    ye, he = dy[:, :, 0::2].contiguous(), dh[:, :, 0].contiguous()
    for nv in (0.3, torch.from_numpy(10.0 ** rng.uniform(-2, 0, B)).cuda()):
        z, nvs = _np(*D.stbc_combine_device(dy, dh, nv, S=S, coh=coh))
        if R == 1:
            ez, env = _np(*D.equalize_device(ye[:, 0].contiguous(), he[:, 0].contiguous(), nv, coh=coh // 2))
        else:
            ez, env = _np(*D.combine_device(ye, he, nv, coh=coh // 2))
        assert np.array_equal(z[:, 0::2], ez) and np.array_equal(nvs[:, 0::2], env)   # IEEE ==


# ---- the generator ----------------------------------------------------------------------------------
_CODECS = {}


def _codec(n, rate, **kw):
    key = (n, rate, tuple(sorted(kw.items())))
    if key not in _CODECS:
        _CODECS[key] = M.DVBRCS2_Turbo(n, rate, interleaver="valid-perm", **kw)
    return _CODECS[key]


def _points(c, info, mod):
    """The table points of the oracle-encoded info bits, complex64 [B, S]."""
    t, G = O.trellis()
    pm = T.puncture_matrix(c.punct)
    coded = np.stack([O.encode(b, c.N, c.punct["period"], pm, c.perm, t, G) for b in info])
    return D.constellation(mod).astype(np.complex64)[GC.labels(coded, D.MODULATIONS[mod]["bps"])]


GEN = dict(n=212, rate="3/4", mod="8PSK", S=195, B=130, seed=0xDEADBEEF12345)   # an odd S: S2 = 196


@pytest.mark.parametrize("K,coh,R,cw0", [(4.0, 14, 3, 2 ** 32 - 40), (0.0, 196, 1, 2 ** 40 + 12345), (0.0, 2, 8, 0)])
def test_generator(K, coh, R, cw0):
    c, mod, B, seed, S = _codec(GEN["n"], GEN["rate"]), GEN["mod"], GEN["B"], GEN["seed"], GEN["S"]
    S2, cw = S + 1, GC.cws(cw0, B)
    assert -(-c.n_coded // 3) == S
    nh = -(-S2 // coh)
    fading = {"K": K, "coh": coh, "branches": R, "tx_antennas": 2}
    gen = lambda n, at, ebn0: W.make_symbols(c, n, mod, ebn0, seed, "cuda", cw0=at, fading=fading)  # noqa: E731
    info, clean, _, h = gen(B, cw0, 1000.0)                           # sigma rounds to 0 in float32
    assert tuple(clean.shape) == (B, R, S2) and tuple(h.shape) == (B, R, 2, nh) and h.dtype == torch.complex64
    # info bits: the generators' own, and the oracle's restatement
    assert torch.equal(info, W.info_bits(c, B, seed, "cuda", cw0=cw0))
    assert np.array_equal(info.cpu().numpy(), WR.info_bits(cw, c.N, seed))
    # antenna 0's gains: sqrt(1/2) in float32 times what the branch generator writes, bit for bit
    _, _, _, hb = W.make_symbols(c, B, mod, 1000.0, seed, "cuda", cw0=cw0, want_info=False,
                                 fading={"K": K, "coh": coh, "branches": R})
    hb, hd = hb.cpu().numpy(), h.cpu().numpy()
    assert hb.shape == (B, R, nh)
    assert _eq(hd[:, :, 0], GC.to_c64(hb.real * SR.SQRT_HALF, hb.imag * SR.SQRT_HALF))
    # antenna 1's: the restatement on the new domain word, within the generator tests' bound
    ref, rad = SR.gains(cw, R, nh, seed, K)
    for a in (0, 1):
        e = SR.gains_excess(hd[:, :, a], ref[:, :, a], rad[:, :, a])
        print(f"antenna {a} gains: worst excess / rad {np.max(e):.3e} (bound {GC.bound():.3e})")
        assert np.all(e <= GC.bound())
    assert not np.array_equal(hd[:, :, 1], hd[:, :, 0])
    # sigma = 0: the stated float32 expression of the written gains and the oracle's table points (IEEE ==: the
    # noise term is a signed zero), the conjugated slots and the pad slot included
    x = _points(c, info.cpu().numpy(), mod)
    assert x.shape == (B, S)
    sig = SR.signal32(hd, x, coh)
    assert np.array_equal(clean.cpu().numpy(), sig)
    # sigma > 0: the same gains, and slots minus that signal inside the noise bound of the restated sample
    _, noisy, n0, h2 = gen(B, cw0, 4.0)
    assert torch.equal(h2, h)
    sigma = float(np.sqrt(n0 / 2))
    nref, nrad = SR.noise(cw, R, S2, seed, sigma)
    e = GC.excess(noisy.cpu().numpy(), sig.astype(np.complex128) + nref, nrad)
    print(f"slots: worst excess / rad {np.max(e):.3e} (bound {GC.bound():.3e})")
    assert np.all(e <= GC.bound())
    # a codeword depends on its global index only: a 64 + 66 split at a moved cw0 equals the batch exactly, gains
    # and info bits included
    a, b = gen(64, cw0, 4.0), gen(66, cw0 + 64, 4.0)
    assert torch.equal(torch.cat([a[1], b[1]]), noisy) and torch.equal(torch.cat([a[3], b[3]]), h)
    assert torch.equal(torch.cat([a[0], b[0]]), info)


def test_one_antenna_is_the_call_without_the_key():
    c = _codec(48, "1/3")
    for fading in ({"K": 4.0, "coh": 5}, {"K": 0.0, "coh": 6, "branches": 2}):
        a = W.make_symbols(c, 70, "16QAM", 3.0, 9, "cuda", fading=fading)
        b = W.make_symbols(c, 70, "16QAM", 3.0, 9, "cuda", fading={**fading, "tx_antennas": 1})
        assert a[2] == b[2] and all(torch.equal(p, q) for p, q in zip((a[0], a[1], a[3]), (b[0], b[1], b[3])))
    # one branch of the 2 x R link: still 3-D / 4-D
    _, s, _, h = W.make_symbols(c, 3, "16QAM", 3.0, 9, "cuda", fading={"K": 0.0, "coh": 6, "tx_antennas": 2})
    assert tuple(s.shape) == (3, 1, 72) and tuple(h.shape) == (3, 1, 2, 12)


# ---- combine -> demap -> decode against the reference chain ---------------------------------------
CHAIN = [(48, "1/3", "QPSK", 8), (212, "1/2", "16QAM", None)]        # coh: slots per gain block (None: S2)
NB = 67


def _llr64(z, nvs, mod):
    cons = D.constellation(mod)
    _, div_f32, _ = D.demap_mode(np.complex64, cons.dtype, np.float64(1.0))
    return -F.demap_per_symbol(z, cons, D.MODULATIONS[mod]["bps"], nvs, div_f32)    # decoder sign


@pytest.fixture(scope="module")
def chain_ref():
    """Per (N, rate, mod) and R = 1, 2: 67 bursts over a 2 x R Rayleigh link at 4 dB, and the reference
    chain's decoder-sign float64 LLRs: restated combiner -> oracle.demap per symbol.  Computed once."""
    out = {}
    for n, rate, mod, coh in CHAIN:
        c = _codec(n, rate)
        S = -(-c.n_coded // D.MODULATIONS[mod]["bps"])
        coh = coh or SR.s2_of(S)
        for R in (1, 2):
            fading = {"K": 0.0, "coh": coh, "branches": R, "tx_antennas": 2}
            _, syms, n0, h = W.make_symbols(c, NB, mod, 4.0, 77, "cuda", want_info=False, fading=fading)
            z, nvs = SR.combine(syms.cpu().numpy(), h.cpu().numpy(), n0, S, coh)
            out[(n, R)] = dict(syms=syms, h=h, n0=n0, S=S, coh=coh, z=z, nvs=nvs, llr=_llr64(z, nvs, mod))
    return out


def _oracle(c, llr):
    t, _ = O.trellis()
    return O.decode_batch(llr[:, :c.n_coded].astype(np.float32), c.N, c.punct["period"], T.puncture_matrix(c.punct),
                          c.iterations, c.perm, c.inv_perm, t, want_lfinal=True)


def _lfinal(c, pipe, n):
    """L_final of the planes the pipeline's last batch demapped."""
    bits = torch.empty((n, c.k_info), dtype=torch.int32, device="cuda")
    lf = torch.empty((n, c.k_info), dtype=torch.float64, device="cuda")
    c.decode_planes_device(pipe.planes, n, bits, lfinal=lf)
    return bits.cpu().numpy(), lf.cpu().numpy()


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("n,rate,mod,_coh", CHAIN)
def test_run_equals_the_reference_chain(chain_ref, n, rate, mod, _coh, R):
    c, k = _codec(n, rate), chain_ref[(n, R)]
    dev = torch.device("cuda", 0)
    pipe = W.DevicePipeline(c, mod, NB, dev, csi=True)
    want, want_lf = _oracle(c, k["llr"])
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        bits = pipe.run(k["syms"], k["n0"], stream=st, csi=k["h"], coh=k["coh"]).clone()
    st.synchronize()
    assert _eq(pipe.z[:NB].cpu().numpy(), k["z"]) and _eq(pipe.nv_sym[:NB].cpu().numpy(), k["nvs"])
    assert np.array_equal(bits.cpu().numpy(), want) and 0 < int((want != 0).sum())
    b2, lf = _lfinal(c, pipe, NB)
    assert np.array_equal(b2, want) and np.array_equal(lf, want_lf)
    nv_rows = torch.full((NB,), float(k["n0"]), dtype=torch.float64, device=dev)
    assert torch.equal(pipe.run(k["syms"], nv_rows, csi=k["h"], coh=k["coh"]), bits)
    # a shorter batch through the same buffers
    assert torch.equal(pipe.run(k["syms"][:5], k["n0"], csi=k["h"][:5], coh=k["coh"]), bits[:5])


@pytest.mark.parametrize("n,rate,mod,_coh", CHAIN)
def test_early_stop_counts(chain_ref, n, rate, mod, _coh):
    c, k = _codec(n, rate, early_stop=True, es_decoder="tile"), chain_ref[(n, 2)]
    t, _ = O.trellis()
    llr = k["llr"][:, :c.n_coded].astype(np.float32)
    want_bits, _, want_iters = ES.decode_early_stop_batch(llr, c.N, c.punct, c.iterations, c.perm, c.inv_perm, t)
    pipe = W.DevicePipeline(c, mod, NB, torch.device("cuda", 0), csi=True)
    bits = pipe.run(k["syms"], k["n0"], csi=k["h"], coh=k["coh"])
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    assert np.array_equal(pipe.n_iter[:NB].cpu().numpy(), want_iters)
    assert want_iters.min() < c.iterations


@pytest.mark.parametrize("n,rate,mod,_coh", CHAIN)
def test_int8_link(chain_ref, n, rate, mod, _coh):
    """llr="int8": the same chain with the float64 LLRs through tests/llrq_ref.py's quantiser and back."""
    c, k = _codec(n, rate), chain_ref[(n, 2)]
    q = LQ.quantize(k["llr"])
    want, _ = _oracle(c, LQ.dequantize_i8(q))
    pipe = W.DevicePipeline(c, mod, NB, torch.device("cuda", 0), csi=True, llr="int8")
    bits = pipe.run(k["syms"], k["n0"], csi=k["h"], coh=k["coh"])
    assert np.array_equal(pipe.llr_q[:q.size].cpu().numpy().reshape(q.shape), q)
    assert np.array_equal(bits.cpu().numpy(), want)


def test_two_and_three_dimensional_inputs_are_unchanged():
    """run() with 2-D symbols and 2-D gains, and with 3-D symbols and 3-D gains, makes the calls it made:
    equalize_device / combine_device -> demap -> decode, compared with those calls made here directly."""
    n, rate, mod, _ = CHAIN[1]
    c = _codec(n, rate)
    cons, bps = D.constellation(mod), D.MODULATIONS[mod]["bps"]
    div32 = D.demap_mode(np.complex64, cons.dtype, np.float64(1.0))[1]
    S = -(-c.n_coded // bps)

    def decode(z, nvs):
        planes = torch.empty(c.planes_bytes(NB) // 4, dtype=torch.float32, device="cuda")
        c.demap_planes_device(z, cons, bps, nvs, planes, div_f32=div32)
        bits = torch.empty((NB, c.k_info), dtype=torch.int32, device="cuda")
        c.decode_planes_device(planes, NB, bits)
        return bits
    pipe = W.DevicePipeline(c, mod, NB, torch.device("cuda", 0), csi=True)
    _, syms, n0, h = W.make_symbols(c, NB, mod, 4.0, 77, "cuda", want_info=False, fading={"K": 0.0, "coh": S})
    assert syms.dim() == 2 and h.dim() == 2
    assert torch.equal(pipe.run(syms, n0, csi=h, coh=S), decode(*D.equalize_device(syms, h, n0, coh=S)))
    _, syms, n0, h = W.make_symbols(c, NB, mod, 4.0, 77, "cuda", want_info=False,
                                    fading={"K": 0.0, "coh": S, "branches": 2})
    assert syms.dim() == 3 and h.dim() == 3
    assert torch.equal(pipe.run(syms, n0, csi=h, coh=S), decode(*D.combine_device(syms, h, n0, coh=S)))


# ---- refusals ---------------------------------------------------------------------------------------
def test_abi_refusals_write_nothing():
    L, EINVAL = N.lib(), N.TDEC_EINVAL
    B, R, S = 3, 2, 8
    p = N.ptr
    y = torch.ones((B, R, S), dtype=torch.complex64, device="cuda")
    hh = torch.ones((B, R, 2, S // 2), dtype=torch.complex64, device="cuda")
    z = torch.full((B, S), np.nan, dtype=torch.complex64, device="cuda")
    nvs = torch.full((B, S), np.nan, dtype=torch.float64, device="cuda")
    nvr = torch.full((B,), 0.1, dtype=torch.float64, device="cuda")
    nvb = torch.full((B, R), 0.1, dtype=torch.float64, device="cuda")
    good = dict(y=p(y), h=p(hh), B=B, R=R, S=S, coh=2, nv=0.1, rows=None, br=None, z=p(z), nvs=p(nvs))

    def call(**kw):
        a = {**good, **kw}
        return L.stbc_combine_dev(0, a["y"], a["h"], a["B"], a["R"], a["S"], a["coh"], a["nv"], a["rows"], a["br"], a["z"],
                                  a["nvs"], None)
    for kw in (dict(y=None), dict(h=None), dict(z=None), dict(nvs=None), dict(B=-1), dict(S=-1), dict(coh=0), dict(coh=1),
               dict(coh=3), dict(coh=-2), dict(R=0), dict(R=9), dict(R=-1), dict(rows=p(nvr), br=p(nvb)), dict(R=9, B=0),
               dict(coh=1, S=0)):
        assert call(**kw) == EINVAL and "stbc combine" in L.tdec_last_error().decode(), kw
    assert call(B=0, y=None, h=None, z=None, nvs=None) == 0
    assert call(S=0, y=None, h=None, z=None, nvs=None) == 0
    # the generator
    c = _codec(48, "1/3")
    tab = np.ascontiguousarray(D.constellation("16QAM").astype(np.complex64)).view(np.float32)
    Sw = -(-c.handle.enc_len // 4)
    sy = torch.full((B, R, Sw), np.nan, dtype=torch.complex64, device="cuda")
    sh = torch.full((B, R, 2, Sw // 2), np.nan, dtype=torch.complex64, device="cuda")
    wl = L.stbc_workload_dev
    for r_, k_, coh, syms, gains, cw0 in ((0, 0.0, 2, sy, sh, 0), (9, 0.0, 2, sy, sh, 0), (R, -1.0, 2, sy, sh, 0),
                                          (R, np.nan, 2, sy, sh, 0), (R, 0.0, 0, sy, sh, 0), (R, 0.0, 1, sy, sh, 0),
                                          (R, 0.0, 3, sy, sh, 0), (R, 0.0, 2, sy, None, 0), (R, 0.0, 2, None, sh, 0),
                                          (R, 0.0, 2, sy, sh, -1)):
        assert wl(c.handle.h, B, r_, cw0, 1, p(tab), 16, 4, 0.1, k_, coh, p(syms), p(gains), None, None) == EINVAL
    assert wl(None, B, R, 0, 1, p(tab), 16, 4, 0.1, 0.0, 2, p(sy), p(sh), None, None) == EINVAL
    assert wl(c.handle.h, 0, R, 0, 1, p(tab), 16, 4, 0.1, 0.0, 2, None, None, None, None) == 0
    torch.cuda.synchronize()
    for t in (z, sy, sh):
        assert bool(torch.isnan(t.real).all())
    assert bool(torch.isnan(nvs).all())


def test_python_refusals():
    c = _codec(48, "1/3")
    dev = torch.device("cuda", 0)
    two = {"K": 0.0, "coh": 4, "branches": 2, "tx_antennas": 2}
    for fading, kw in (({**two, "coh": 5}, {}), ({**two, "tx_antennas": 3}, {}), ({**two, "branches": 9}, {}),
                       (two, {"pilots": D.PilotLayout(2, 8)}), (two, {"tx": 1}), (two, {"crc": "crc16"})):
        with pytest.raises(ValueError):
            W.make_symbols(c, 4, "QPSK", 3.0, 1, "cuda", fading=fading, **kw)
    _, syms, n0, h = W.make_symbols(c, 4, "QPSK", 3.0, 1, "cuda", want_info=False, fading=two)
    with pytest.raises(ValueError, match="fused"):
        W.DevicePipeline(c, "QPSK", 4, dev, fused=True, csi=True).run(syms, n0, csi=h, coh=4)
    with pytest.raises(ValueError, match="csi=True"):
        W.DevicePipeline(c, "QPSK", 4, dev).run(syms, n0, csi=h, coh=4)
    pipe = W.DevicePipeline(c, "QPSK", 4, dev, csi=True)
    with pytest.raises(ValueError, match="even coh"):
        pipe.run(syms, n0, csi=h, coh=3)
    with pytest.raises(ValueError, match="slots"):
        pipe.run(syms[:, 0].contiguous(), n0, csi=h, coh=4)
    with pytest.raises(ValueError, match="two transmit antennas"):
        pipe.run_frames(syms, D.PilotLayout(2, 8), n0, csi=h)
    with pytest.raises(ValueError):
        D.stbc_combine_device(syms, h, n0, coh=3)
    with pytest.raises(ValueError):
        D.stbc_combine_device(syms, h, n0, S=syms.shape[2] - 2, coh=4)
    with pytest.raises(ValueError):
        D.stbc_combine_device(syms, h[:, :, :1].contiguous(), n0, coh=4)
