"""Spatial multiplexing on the device (include/sm.h): the joint detector
against its numpy restatement (tests/sm_ref.py), the generator's multiplexed 2 x R link, and the
chain detect -> de-puncture -> decode against the restated detector and the oracle.

Every comparison of the detector is IEEE == on the float32 bits (no NaN is ever written).  The
shapes (B, R, S, coh): one symbol (an odd S: the single-stream slot alone); one slot; an odd S over
several rows and branches with a short last gain block; more rows than a workgroup's slots; the
most branches with an odd S, a slot count that fills no wave and one gain block per burst; the
longest row, with a last gain block shorter than coh."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import early_stop_ref as ES  # noqa: E402
import generator_cases as GC  # noqa: E402
import llrq_ref as LQ  # noqa: E402
import sm_ref as SM  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import workload_ref as WR  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

SHAPES = [(1, 1, 1, 1), (2, 1, 2, 1), (3, 2, 7, 2), (65, 3, 72, 4), (4, 8, 145, 73), (2, 4, 564, 24)]
NOISE = ["scalar", "rows", "branches"]
CASES = [(mod, *s) for mod in ("BPSK", "QPSK", "8PSK", "16QAM") for s in SHAPES] + [("64QAM", *s) for s in SHAPES[:4]]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.shape == b.shape and a.dtype == b.dtype == np.float32 and not np.isnan(a).any()
            and np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def _cn(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)


def _data(B, R, S, coh, seed=0):
    """y [B, R, T] and h [B, R, 2, nh] around unit scale with a few decades of spread (so that the LLRs are
    not all at the clip), zero, denormal, huge and non-finite gains and slots sprinkled in."""
    rng = np.random.default_rng(B * S + R + coh + seed)
    Tn = SM.slots_of(S)
    nh = -(-Tn // coh)
    y = (_cn(rng, B, R, Tn) * np.float32(2) ** rng.integers(-3, 2, (B, R, Tn))).astype(np.complex64)
    h = (_cn(rng, B, R, 2, nh) * np.float32(2) ** rng.integers(-4, 1, (B, R, 2, nh))).astype(np.complex64)
    sh = np.array([0, 1e-42 + 3e-43j, np.nan + 1j, 1 + np.inf * 1j, -np.inf, 1e25 - 1e25j, 1e-30j], np.complex64)
    sy = np.array([np.nan, np.inf + 1j, 1 - np.inf * 1j, 0, 1e38 + 1e38j, 1e-44, complex(-0.0, -0.0)], np.complex64)
    hf, yf = h.reshape(-1), y.reshape(-1)
    if hf.size > 8:
        hi = rng.permutation(hf.size)[:len(sh)]
        hf[hi] = sh[:len(hi)]
    if yf.size > 8:
        yi = rng.permutation(yf.size)[:len(sy)]
        yf[yi] = sy[:len(yi)]
    return rng, y, h


def _nv(kind, B, R, rng):
    if kind == "scalar":
        return 0.371
    return 10.0 ** rng.uniform(-2, 0.5, B if kind == "rows" else (B, R))


def _dev(nv):
    return torch.from_numpy(nv).cuda() if isinstance(nv, np.ndarray) else nv


def _rows(nv, sl):
    return nv[sl] if isinstance(nv, np.ndarray) else nv


# ---- the detector ---------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("mod,B,R,S,coh", CASES, ids=lambda v: str(v))
def test_kernel_equals_its_numpy_restatement(mod, B, R, S, coh, noise):
    rng, y, h = _data(B, R, S, coh)
    nv = _nv(noise, B, R, rng)
    cons, bps = D.constellation(mod), D.MODULATIONS[mod]["bps"]
    sign = -1 if (B + R) % 2 else +1
    llr = D.sm_detect_device(torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(), mod, _dev(nv), S=S, coh=coh, sign=sign)
    assert llr.dtype == torch.float32 and tuple(llr.shape) == (B, S * bps)
    ref = SM.detect(y, h, cons, nv, S, coh, sign)
    got = llr.cpu().numpy()
    assert _eq(got, ref)
    if B * S > 8:
        assert (np.abs(ref) < 30).mean() > 0.2 and (ref != 0).mean() > 0.5     # the comparison is not of clipped values alone


@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("mod,B,R,S,coh", [("QPSK", 3, 2, 7, 2), ("16QAM", 65, 3, 72, 4), ("8PSK", 4, 8, 145, 73),
                                           ("64QAM", 3, 2, 7, 2)], ids=lambda v: str(v))
def test_strides_views_and_rows_alone(mod, B, R, S, coh, noise):
    """A row stride above S * bps with guard elements between the rows and behind the last one; y and h one
    element into their buffers; then single bursts (B = 1) against the batch's rows."""
    rng, y, h = _data(B, R, S, coh, seed=1)
    nv = _nv(noise, B, R, rng)
    cons, bps = D.constellation(mod), D.MODULATIONS[mod]["bps"]
    L, pad = S * bps, 5
    ref = SM.detect(y, h, cons, nv, S, coh, -1)
    ybuf = torch.zeros(y.size + 1, dtype=torch.complex64, device="cuda")
    hbuf = torch.zeros(h.size + 1, dtype=torch.complex64, device="cuda")
    ybuf[1:], hbuf[1:] = torch.from_numpy(y).cuda().reshape(-1), torch.from_numpy(h).cuda().reshape(-1)
    dy, dh = ybuf[1:].view(y.shape), hbuf[1:].view(h.shape)
    wide = torch.full((B, L + pad), 77.0, dtype=torch.float32, device="cuda")
    out = wide[:, :L]
    assert D.sm_detect_device(dy, dh, mod, _dev(nv), S=S, coh=coh, out=out, sign=-1) is out
    got = wide.cpu().numpy()
    assert _eq(got[:, :L], ref) and np.all(got[:, L:] == 77.0)
    for b in sorted({0, B // 2, B - 1}):
        one = D.sm_detect_device(dy[b:b + 1].contiguous(), dh[b:b + 1].contiguous(), mod, _dev(_rows(nv, slice(b, b + 1))),
                                 S=S, coh=coh, sign=-1)
        assert _eq(one.cpu().numpy(), ref[b:b + 1])


@pytest.mark.parametrize("sign", [+1, -1])
def test_dead_branches_erasures_and_special_noise(sign):
    rng = np.random.default_rng(5)
    B, R, Tn, coh, mod = 8, 2, 10, 2, "16QAM"
    cons, bps = D.constellation(mod), 4
    y, h = _cn(rng, B, R, Tn), np.float32(0.5) * _cn(rng, B, R, 2, Tn // coh)
    h[0, 1, 0, 2] = np.nan                                            # one branch dead in one block, by a NaN gain
    y[1, 0, 3] = complex(np.nan, 0.0)                                 # ... in one slot, by a NaN y
    y[2, :, 4] = np.inf                                               # all branches dead in one slot: an erasure
    h[3] = np.nan                                                     # a whole row of erasures
    h[4] = 0                                                          # zero gains are live: signed zeros
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    rows = np.array([0.3, 0.001, np.nan, 0.3, 0.3, np.inf, 0.0, 2.0])
    br = np.stack([rows, rows[::-1]], axis=1)
    for nv in (0.3, 0.001, np.nan, np.inf, rows, br):
        got = D.sm_detect_device(dy, dh, mod, _dev(nv) if isinstance(nv, np.ndarray) else float(nv), coh=coh,
                                 sign=sign).cpu().numpy()
        assert _eq(got, SM.detect(y, h, cons, nv, coh=coh, sign=sign))
        g = got.reshape(B, Tn, 2 * bps)
        for z in (g[2, 4], g[3]):                                     # erasures: +0.0f whatever the sign
            assert not z.any() and not np.signbit(z).any()
        if isinstance(nv, float) and nv == 0.3:
            assert not g[4].any() and np.all(np.signbit(g[4]) == (sign < 0))
            alone = D.sm_detect_device(dy[:, :1].contiguous(), dh[:, :1].contiguous(), mod, 0.3, coh=coh, sign=sign)
            a = alone.cpu().numpy().reshape(B, Tn, 2 * bps)
            assert _eq(g[0, 4:6], a[0, 4:6]) and not _eq(g[0, 0:2], a[0, 0:2])   # the live branch alone, there only
    floor = D.sm_detect_device(dy, dh, mod, 0.005, coh=coh, sign=sign).cpu().numpy()
    assert _eq(D.sm_detect_device(dy, dh, mod, 0.001, coh=coh, sign=sign).cpu().numpy(), floor)
    assert _eq(D.sm_detect_device(dy, dh, mod, float("nan"), coh=coh, sign=sign).cpu().numpy(), floor)
    assert not D.sm_detect_device(dy, dh, mod, float("inf"), coh=coh, sign=sign).cpu().numpy().any()


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


GEN = dict(n=212, rate="3/4", mod="8PSK", S=195, B=130, seed=0xDEADBEEF12345)   # an odd S: 98 slots, the last single-stream


@pytest.mark.parametrize("K,coh,R,cw0", [(4.0, 7, 3, 2 ** 32 - 40), (0.0, 98, 1, 2 ** 40 + 12345), (0.0, 1, 8, 0)])
def test_generator(K, coh, R, cw0):
    c, mod, B, seed, S = _codec(GEN["n"], GEN["rate"]), GEN["mod"], GEN["B"], GEN["seed"], GEN["S"]
    Tn, cw = SM.slots_of(S), GC.cws(cw0, B)
    assert -(-c.n_coded // 3) == S
    nh = -(-Tn // coh)
    fading = {"K": K, "coh": coh, "branches": R}
    gen = lambda n, at, ebn0: W.make_symbols(c, n, mod, ebn0, seed, "cuda", cw0=at, fading=fading, streams=2)  # noqa: E731
    info, clean, _, h = gen(B, cw0, 1000.0)                           # sigma rounds to 0 in float32
    assert tuple(clean.shape) == (B, R, Tn) and tuple(h.shape) == (B, R, 2, nh) and h.dtype == torch.complex64
    assert torch.equal(info, W.info_bits(c, B, seed, "cuda", cw0=cw0))
    assert np.array_equal(info.cpu().numpy(), WR.info_bits(cw, c.N, seed))
    # the gains are the Alamouti link's, bit for bit: its block j covers slots [j 2 coh', ...) of its own slot
    # count, so compare block by block on a link with the same number of blocks per burst
    hd = h.cpu().numpy()
    _, _, _, hs = W.make_symbols(c, B, mod, 1000.0, seed, "cuda", cw0=cw0, want_info=False,
                                 fading={**fading, "coh": 2, "tx_antennas": 2})
    hs = hs.cpu().numpy()                                             # [B, R, 2, 98]: block j is draw j
    assert hs.shape[3] >= nh and np.array_equal(hd.view(np.uint32), np.ascontiguousarray(hs[:, :, :, :nh]).view(np.uint32))
    ref, rad = SM.gains(cw, R, nh, seed, K)
    for a in (0, 1):
        e = SM.gains_excess(hd[:, :, a], ref[:, :, a], rad[:, :, a])
        print(f"antenna {a} gains: worst excess / rad {np.max(e):.3e} (bound {GC.bound():.3e})")
        assert np.all(e <= GC.bound())
    # sigma = 0: the stated float32 expression of the written gains and the oracle's table points (IEEE ==: the
    # noise term is a signed zero), the single-stream slot included
    x = _points(c, info.cpu().numpy(), mod)
    assert x.shape == (B, S)
    sig = SM.signal32(hd, x, coh)
    assert np.array_equal(clean.cpu().numpy(), sig)
    # sigma > 0: the same gains, and slots minus that signal inside the noise bound of the restated sample
    _, noisy, n0, h2 = gen(B, cw0, 4.0)
    assert torch.equal(h2, h)
    sigma = float(np.sqrt(n0 / 2))
    nref, nrad = SM.noise(cw, R, Tn, seed, sigma)
    e = GC.excess(noisy.cpu().numpy(), sig.astype(np.complex128) + nref, nrad)
    print(f"slots: worst excess / rad {np.max(e):.3e} (bound {GC.bound():.3e})")
    assert np.all(e <= GC.bound())
    # a codeword depends on its global index only: a 64 + 66 split at a moved cw0 equals the batch exactly
    a, b = gen(64, cw0, 4.0), gen(66, cw0 + 64, 4.0)
    assert torch.equal(torch.cat([a[1], b[1]]), noisy) and torch.equal(torch.cat([a[3], b[3]]), h)
    assert torch.equal(torch.cat([a[0], b[0]]), info)


def test_one_stream_is_the_call_without_the_keyword():
    c = _codec(48, "1/3")
    for fading in ({"K": 4.0, "coh": 5}, {"K": 0.0, "coh": 6, "branches": 2}, {"K": 0.0, "coh": 6, "tx_antennas": 2}):
        a = W.make_symbols(c, 70, "16QAM", 3.0, 9, "cuda", fading=fading)
        b = W.make_symbols(c, 70, "16QAM", 3.0, 9, "cuda", fading=fading, streams=1)
        assert a[2] == b[2] and all(torch.equal(p, q) for p, q in zip((a[0], a[1], a[3]), (b[0], b[1], b[3])))
    _, s, _, h = W.make_symbols(c, 3, "16QAM", 3.0, 9, "cuda", fading={"K": 0.0, "coh": 5}, streams=2)
    assert tuple(s.shape) == (3, 1, 36) and tuple(h.shape) == (3, 1, 2, 8)


# ---- detect -> de-puncture -> decode against the restated detector and the oracle -----------------
CHAIN = [(48, "1/3", "QPSK", 8), (212, "1/2", "16QAM", None)]        # coh: slots per gain block (None: T)
NB = 67


@pytest.fixture(scope="module")
def chain_ref():
    """Per (N, rate, mod) and R = 1, 2: 67 bursts over a multiplexed 2 x R Rayleigh link, and the restated
    detector's decoder-sign float32 LLRs.  Computed once."""
    out = {}
    for n, rate, mod, coh in CHAIN:
        c = _codec(n, rate)
        S = -(-c.n_coded // D.MODULATIONS[mod]["bps"])
        coh = coh or SM.slots_of(S)
        for R in (1, 2):
            fading = {"K": 0.0, "coh": coh, "branches": R}
            _, y, n0, h = W.make_symbols(c, NB, mod, 9.0 if R == 1 else 6.0, 77, "cuda", want_info=False, fading=fading,
                                         streams=2)
            llr = SM.detect(y.cpu().numpy(), h.cpu().numpy(), D.constellation(mod), n0, S, coh, -1)
            out[(n, R)] = dict(y=y, h=h, n0=n0, S=S, coh=coh, llr=llr)
    return out


def _oracle(c, llr):
    t, _ = O.trellis()
    return O.decode_batch(np.ascontiguousarray(llr[:, :c.n_coded], np.float32), c.N, c.punct["period"],
                          T.puncture_matrix(c.punct), c.iterations, c.perm, c.inv_perm, t, want_lfinal=True)


def _lfinal(c, pipe, n):
    """L_final of the planes the pipeline's last batch wrote."""
    bits = torch.empty((n, c.k_info), dtype=torch.int32, device="cuda")
    lf = torch.empty((n, c.k_info), dtype=torch.float64, device="cuda")
    c.decode_planes_device(pipe.planes, n, bits, lfinal=lf)
    return bits.cpu().numpy(), lf.cpu().numpy()


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("n,rate,mod,_coh", CHAIN)
def test_run_sm_equals_the_reference_chain(chain_ref, n, rate, mod, _coh, R):
    c, k = _codec(n, rate), chain_ref[(n, R)]
    dev = torch.device("cuda", 0)
    pipe = W.DevicePipeline(c, mod, NB, dev, sm=True)
    want, want_lf = _oracle(c, k["llr"])
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        bits = pipe.run_sm(k["y"], k["n0"], k["h"], coh=k["coh"], stream=st).clone()
    st.synchronize()
    assert _eq(pipe.llr_sm[:NB].cpu().numpy(), k["llr"])
    assert np.array_equal(bits.cpu().numpy(), want) and 0 < int((want != 0).sum())
    b2, lf = _lfinal(c, pipe, NB)
    assert np.array_equal(b2, want) and np.array_equal(lf, want_lf)
    nv_rows = torch.full((NB,), float(k["n0"]), dtype=torch.float64, device=dev)
    assert torch.equal(pipe.run_sm(k["y"], nv_rows, k["h"], coh=k["coh"]), bits)
    assert torch.equal(pipe.run_sm(k["y"][:5], k["n0"], k["h"][:5], coh=k["coh"]), bits[:5])   # a shorter batch


@pytest.mark.parametrize("n,rate,mod,_coh", CHAIN)
def test_early_stop_counts(chain_ref, n, rate, mod, _coh):
    c, k = _codec(n, rate, early_stop=True, es_decoder="tile"), chain_ref[(n, 2)]
    t, _ = O.trellis()
    llr = np.ascontiguousarray(k["llr"][:, :c.n_coded], np.float32)
    want_bits, _, want_iters = ES.decode_early_stop_batch(llr, c.N, c.punct, c.iterations, c.perm, c.inv_perm, t)
    pipe = W.DevicePipeline(c, mod, NB, torch.device("cuda", 0), sm=True)
    bits = pipe.run_sm(k["y"], k["n0"], k["h"], coh=k["coh"])
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    assert np.array_equal(pipe.n_iter[:NB].cpu().numpy(), want_iters)
    assert want_iters.min() < c.iterations


@pytest.mark.parametrize("n,rate,mod,_coh", CHAIN)
def test_int8_link(chain_ref, n, rate, mod, _coh):
    """llr="int8": the same chain with the restated LLRs through tests/llrq_ref.py's quantiser and back."""
    c, k = _codec(n, rate), chain_ref[(n, 2)]
    q = LQ.quantize(k["llr"])
    want, _ = _oracle(c, LQ.dequantize_i8(q))
    pipe = W.DevicePipeline(c, mod, NB, torch.device("cuda", 0), sm=True, llr="int8")
    bits = pipe.run_sm(k["y"], k["n0"], k["h"], coh=k["coh"])
    assert np.array_equal(pipe.llr_q[:q.size].cpu().numpy().reshape(q.shape), q)
    assert np.array_equal(bits.cpu().numpy(), want)


def test_a_noise_free_burst_decodes_to_its_info_bits():
    """R = 2, sigma = 0 (Eb/N0 = 1000 dB rounds to it in float32), interleaver="valid-perm".  The seed is first
    checked on the CPU to decode in the restated chain -- a condition on the input, not a tolerance."""
    n, rate, mod, _ = CHAIN[1]
    c = _codec(n, rate)
    S = -(-c.n_coded // 4)
    coh = SM.slots_of(S)
    info, y, n0, h = W.make_symbols(c, 16, mod, 1000.0, 2024, "cuda", fading={"K": 0.0, "coh": coh, "branches": 2}, streams=2)
    llr = SM.detect(y.cpu().numpy(), h.cpu().numpy(), D.constellation(mod), n0, S, coh, -1)
    want, _ = _oracle(c, llr)
    assert np.array_equal(want, info.cpu().numpy())                   # the input's condition
    pipe = W.DevicePipeline(c, mod, 16, torch.device("cuda", 0), sm=True)
    assert torch.equal(pipe.run_sm(y, n0, h, coh=coh), info.to(torch.int32))


def test_run_is_untouched_by_a_pipeline_built_with_sm():
    """run() of a pipeline built with sm=True makes the calls it made: 2-D symbols through the plane demapper."""
    n, rate, mod, _ = CHAIN[0]
    c = _codec(n, rate)
    _, syms, n0 = W.make_symbols(c, NB, mod, 4.0, 3, "cuda", want_info=False)
    dev = torch.device("cuda", 0)
    assert torch.equal(W.DevicePipeline(c, mod, NB, dev, sm=True).run(syms, n0), W.DevicePipeline(c, mod, NB, dev).run(syms, n0))


# ---- refusals ---------------------------------------------------------------------------------------
def test_abi_refusals_write_nothing():
    L, EINVAL = N.lib(), N.TDEC_EINVAL
    B, R, S, bps = 3, 2, 8, 2
    p = N.ptr
    y = torch.ones((B, R, S // 2), dtype=torch.complex64, device="cuda")
    hh = torch.ones((B, R, 2, S // 2), dtype=torch.complex64, device="cuda")
    llr = torch.full((B, S * bps), np.nan, dtype=torch.float32, device="cuda")
    nvr = torch.full((B,), 0.1, dtype=torch.float64, device="cuda")
    nvb = torch.full((B, R), 0.1, dtype=torch.float64, device="cuda")
    tab = np.ascontiguousarray(D.constellation("QPSK"))
    assert tab.dtype == np.complex128
    good = dict(y=p(y), h=p(hh), B=B, R=R, S=S, coh=1, cons=p(tab), M=4, nv=0.1, rows=None, br=None, llr=p(llr),
                stride=S * bps)

    def call(**kw):
        a = {**good, **kw}
        return L.sm_detect_dev(0, a["y"], a["h"], a["B"], a["R"], a["S"], a["coh"], a["cons"], 1, a["M"], a["nv"], a["rows"],
                               a["br"], -1, a["llr"], a["stride"], None)
    for kw in (dict(y=None), dict(h=None), dict(cons=None), dict(llr=None), dict(B=-1), dict(S=-1), dict(coh=0), dict(coh=-2),
               dict(R=0), dict(R=9), dict(R=-1), dict(M=1), dict(M=0), dict(M=3), dict(M=48), dict(M=128), dict(M=256),
               dict(stride=S * bps - 1), dict(stride=0), dict(rows=p(nvr), br=p(nvb)), dict(R=9, B=0), dict(coh=0, S=0)):
        assert call(**kw) == EINVAL and "sm detect" in L.tdec_last_error().decode(), kw
    for bad in (np.inf, -np.inf, np.nan, 1.0000001e30, -2e30):         # a table component outside [-1e30, 1e30]
        t2 = tab.copy()
        t2.view(np.float64)[5] = bad
        assert call(cons=p(t2)) == EINVAL and "table components" in L.tdec_last_error().decode(), bad
    t2 = tab.copy()
    t2.view(np.float64)[5] = -1e30                                     # the bound itself is taken
    assert call(cons=p(t2)) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(llr).any())
    llr.fill_(np.nan)
    # an empty batch is a no-op before any pointer is looked at, the table's included; the sizes are checked first
    assert call(B=0, y=None, h=None, llr=None, cons=None) == 0
    assert call(S=0, y=None, h=None, llr=None, cons=None, stride=0) == 0
    # the generator
    c = _codec(48, "1/3")
    tab32 = np.ascontiguousarray(D.constellation("16QAM").astype(np.complex64)).view(np.float32)
    Tw = -(-c.handle.enc_len // 4) // 2
    sy = torch.full((B, R, Tw), np.nan, dtype=torch.complex64, device="cuda")
    sh = torch.full((B, R, 2, Tw), np.nan, dtype=torch.complex64, device="cuda")
    wl = L.sm_workload_dev
    for r_, k_, coh, syms, gains, cw0 in ((0, 0.0, 1, sy, sh, 0), (9, 0.0, 1, sy, sh, 0), (R, -1.0, 1, sy, sh, 0),
                                          (R, np.nan, 1, sy, sh, 0), (R, 0.0, 0, sy, sh, 0), (R, 0.0, -1, sy, sh, 0),
                                          (R, 0.0, 1, sy, None, 0), (R, 0.0, 1, None, sh, 0), (R, 0.0, 1, sy, sh, -1)):
        assert wl(c.handle.h, B, r_, cw0, 1, p(tab32), 16, 4, 0.1, k_, coh, p(syms), p(gains), None, None) == EINVAL
    assert wl(None, B, R, 0, 1, p(tab32), 16, 4, 0.1, 0.0, 1, p(sy), p(sh), None, None) == EINVAL
    assert wl(c.handle.h, 0, R, 0, 1, p(tab32), 16, 4, 0.1, 0.0, 1, None, None, None, None) == 0
    torch.cuda.synchronize()
    for t in (sy, sh):
        assert bool(torch.isnan(t.real).all())
    assert bool(torch.isnan(llr).all())


def test_python_refusals():
    c = _codec(48, "1/3")
    dev = torch.device("cuda", 0)
    f = {"K": 0.0, "coh": 3, "branches": 2}
    for fading, kw in ((None, {}), ({**f, "tx_antennas": 2, "coh": 4}, {}), ({**f, "branches": 9}, {}), ({**f, "coh": 0}, {}),
                       (f, {"pilots": D.PilotLayout(2, 8)}), (f, {"tx": 1}), (f, {"crc": "crc16"})):
        with pytest.raises(ValueError):
            W.make_symbols(c, 4, "QPSK", 3.0, 1, "cuda", fading=fading, streams=2, **kw)
    with pytest.raises(ValueError, match="64-point"):
        W.make_symbols(c, 4, "256QAM", 3.0, 1, "cuda", fading=f, streams=2)
    _, y, n0, h = W.make_symbols(c, 4, "QPSK", 3.0, 1, "cuda", want_info=False, fading=f, streams=2)
    for kw in ({"fused": True}, {"overlap": True}, {"demap": "log-map"}):
        with pytest.raises(ValueError, match="sm=True"):
            W.DevicePipeline(c, "QPSK", 4, dev, sm=True, **kw)
    with pytest.raises(ValueError, match="64-point"):
        W.DevicePipeline(c, "256QAM", 4, dev, sm=True)
    with pytest.raises(ValueError, match="sm=True"):
        W.DevicePipeline(c, "QPSK", 4, dev).run_sm(y, n0, h, coh=3)
    pipe = W.DevicePipeline(c, "QPSK", 4, dev, sm=True)
    with pytest.raises(ValueError, match="slots"):
        pipe.run_sm(y[:, :, :-1].contiguous(), n0, h, coh=3)
    with pytest.raises(ValueError, match="coh"):
        pipe.run_sm(y, n0, h, coh=0)
    with pytest.raises(ValueError):
        pipe.run_sm(y, n0, h, coh=4)                                  # h has ceil(T / 3) blocks
    with pytest.raises(ValueError):
        D.sm_detect_device(y, h, "QPSK", n0, S=2 * y.shape[2] - 2, coh=3)
    with pytest.raises(ValueError):
        D.sm_detect_device(y, h[:, :, :1].contiguous(), "QPSK", n0, coh=3)
    with pytest.raises(ValueError, match="sign"):
        D.sm_detect_device(y, h, "QPSK", n0, coh=3, sign=0)
    with pytest.raises(ValueError, match="out"):
        D.sm_detect_device(y, h, "QPSK", n0, coh=3, out=torch.empty((4, 2 * y.shape[2] * 2), dtype=torch.float64, device=dev))
    with pytest.raises(TypeError):
        D.sm_detect_device(y, h, "QPSK", torch.ones(4, dtype=torch.float32, device=dev), coh=3)


# ---- a 32-point table through the ABI, the f16 link, the sweep -----------------------------------------
@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("B,R,S,coh", [(3, 2, 7, 2), (5, 3, 72, 4)], ids=lambda v: str(v))
def test_a_32_point_table_through_the_abi(B, R, S, coh, f64, noise):
    """No modulation of the package has 32 points, the ABI takes any power of two up to 64: k_sm_detect<32, *>
    (two unrolled blocks of 16 and one high label bit) against the restatement on a made-up table, float32
    and float64."""
    rng, y, h = _data(B, R, S, coh, seed=32)
    nv = _nv(noise, B, R, rng)
    tab = (rng.standard_normal(32) + 1j * rng.standard_normal(32)) * 0.8
    tab = np.ascontiguousarray(tab.astype(np.complex128 if f64 else np.complex64))
    ref = SM.detect(y, h, tab, nv, S, coh, -1)
    assert ref.shape == (B, S * 5) and (np.abs(ref) < 30).mean() > 0.2
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    out = torch.full((B, S * 5), np.nan, dtype=torch.float32, device="cuda")
    dn = _dev(nv)
    p = N.ptr
    rc = N.lib().sm_detect_dev(0, p(dy), p(dh), B, R, S, coh, p(tab), int(f64), 32, nv if noise == "scalar" else 0.0,
                               p(dn) if noise == "rows" else None, p(dn) if noise == "branches" else None, -1, p(out),
                               S * 5, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert _eq(out.cpu().numpy(), ref)


@pytest.mark.parametrize("n,rate,mod,_coh", CHAIN)
def test_f16_link(chain_ref, n, rate, mod, _coh):
    """llr="f16": the detector's float32 LLRs rounded once to float16 (numpy's astype rounds to nearest even, as
    the device copy does) and widened by the de-puncture kernel, tests/llrq_ref.py's dequantize_f16."""
    c, k = _codec(n, rate), chain_ref[(n, 2)]
    q = k["llr"].astype(np.float16)
    want, _ = _oracle(c, LQ.dequantize_f16(q))
    pipe = W.DevicePipeline(c, mod, NB, torch.device("cuda", 0), sm=True, llr="f16")
    bits = pipe.run_sm(k["y"], k["n0"], k["h"], coh=k["coh"])
    got = pipe.llr_q[:q.size].cpu().numpy().reshape(q.shape)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), q.view(np.uint16))
    assert np.array_equal(bits.cpu().numpy(), want)


def test_the_sweep_runs_a_multiplexed_point():
    """python -m modulations_amd.ber --tx-antennas 2 --tx-mode sm, two points of 2048 codewords: the records name
    the mode, and their error counts are those of the same calls made here (make_symbols(streams=2) ->
    run_sm -> count_errors on the sweep's per-point seed).  The far points bracket the link: nearly every
    frame is wrong at -12 dB, nearly none at 30 dB (2 x 2, rate 1/3, one gain per path and burst)."""
    from modulations_amd import ber
    n_cw, seed = 2048, 2025
    args = ["--mod", "QPSK", "--n", "48", "--rate", "1/3", "--interleaver", "valid-perm", "--channel", "rayleigh",
            "--coherence", "72", "--tx-antennas", "2", "--tx-mode", "sm", "--rx-branches", "2", "--codewords", str(n_cw),
            "--batch", "1024", "--seed", str(seed), "--ebn0=-12,30"]
    recs = ber.main(args)
    assert [r["ebn0_db"] for r in recs] == [-12.0, 30.0]
    c = _codec(48, "1/3")
    pipe = W.DevicePipeline(c, "QPSK", 1024, torch.device("cuda", 0), sm=True)
    for r in recs:
        assert r["tx_mode"] == "sm" and r["tx_antennas"] == 2 and r["rx_branches"] == 2 and r["codewords"] == n_cw
        assert r["coherence"] == 72 and r["step_ms"] > 0
        be = fe = 0
        s = ber.ebn0_seed(seed, r["ebn0_db"])
        for off in (0, 1024):
            _, y, n0, h = W.make_symbols(c, 1024, "QPSK", r["ebn0_db"], s, "cuda", cw0=off, want_info=False,
                                         fading={"K": 0.0, "coh": 72, "branches": 2}, streams=2)
            e = W.count_errors(c, pipe.run_sm(y, n0, h, coh=72), s, cw0=off)
            be, fe = be + int(e.sum()), fe + int((e > 0).sum())
        assert (r["bit_errors"], r["frame_errors"]) == (be, fe)
    print("FER at -12 dB", recs[0]["fer"], "at 30 dB", recs[1]["fer"])
    assert recs[0]["fer"] > 0.9 and recs[1]["fer"] < 0.05


def test_a_batch_past_two_to_the_32_threads():
    """A slot takes M threads and one launch holds fewer than 2^32: 64QAM with B * T = 65537 * 1024 slots is
    2^32 + 65536 threads, so the call goes out as two launches, the second starting inside row 65535.  Every LLR
    of the NaN-filled output is overwritten, and the first rows, one in the middle and the last two equal the
    restatement bit for bit."""
    mod, B, Tn, R = "64QAM", 65537, 1024, 1
    assert B * Tn * 64 > 2 ** 32
    gen = torch.Generator(device="cuda").manual_seed(12)
    y = torch.view_as_complex(torch.randn((B, R, Tn, 2), dtype=torch.float32, device="cuda", generator=gen))
    h = torch.view_as_complex(torch.randn((B, R, 2, 1, 2), dtype=torch.float32, device="cuda", generator=gen) * 0.5)
    out = torch.full((B, 2 * Tn * 6), np.nan, dtype=torch.float32, device="cuda")
    D.sm_detect_device(y, h, mod, 0.371, coh=Tn, out=out, sign=-1)
    assert not bool(torch.isnan(out).any())
    rows = [0, 1, 30000, B - 2, B - 1]
    ref = SM.detect(y[rows].cpu().numpy(), h[rows].cpu().numpy(), D.constellation(mod), 0.371, coh=Tn, sign=-1)
    assert _eq(out[rows].cpu().numpy(), ref) and (np.abs(ref) < 30).mean() > 0.2
