"""Flat fading on the device: the per-symbol noise variance of
the five demap kernels, the equaliser, the fading generator and the chain.

The demappers' contract is exact: symbol (r, s) of a per-symbol launch is, bit for bit,
what the scalar launch gives that symbol with noise_var = nv[r, s].  So every demapper
test runs the scalar entry point on the whole batch once per distinct value, takes the
symbols (for the planes: the plane entries fed by the symbols) that carry that value,
and compares bit patterns, NaNs at the same positions included.  Neighbouring symbols
always carry different values, so both symbols of a couple whose label bits straddle
two symbols do.  The equaliser is compared bit for bit with its numpy restatement
(tests/fading_ref.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import early_stop_ref as ES  # noqa: E402
import fading_ref as F  # noqa: E402
import generator_abi as GA  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import workload_ref as WR  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

MODS = ["BPSK", "QPSK", "8PSK", "16QAM", "64QAM", "256QAM"]
PLANE_VALS = [0.001, 0.05, 0.3, 7.0, 1e5]            # below the floor .. above the unscaled division's range
DECLINE_VALS = [0.005, 0.05, 0.3, np.inf, np.nan]
FLAT_VALS = [0.001, 0.3, 1e5, np.nan, np.inf]
B_PLANES = 69                                         # one full 64-lane tile and a partial one


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _scatter(vals, B, S, start=0):
    """[B, S] values of `vals` (5 of them): symbol (r, s) takes vals[(start + r + 2 s) % 5], so
    horizontal neighbours differ (by 2) and so do vertical ones (by 1)."""
    r, s = np.arange(B)[:, None], np.arange(S)[None, :]
    return np.asarray(vals, np.float64)[(start + r + 2 * s) % len(vals)]


def _is(nv, v):
    return np.isnan(nv) if np.isnan(v) else nv == v


_CODECS = {}


def _codec(n, rate, **kw):
    key = (n, rate, tuple(sorted(kw.items())))
    if key not in _CODECS:
        _CODECS[key] = M.DVBRCS2_Turbo(n, rate, **kw)
    return _CODECS[key]


def _noisy(cons, rng, shape, sigma=0.25):
    return (cons[rng.integers(0, len(cons), shape)] +
            sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))).astype(np.complex64)


def _boundary(cons, rng, shape):
    """Mostly noisy points; the rest on exact decision boundaries (midpoints between
    adjacent levels on one axis and on both), NaN, +-inf and 1e30: what the split
    tables' fast search declines and k_demap_fix redoes (the inputs of
    tests/test_gpu_demap_rownv.py)."""
    s = _noisy(cons, rng, shape)
    lv = np.unique(cons.real.astype(np.float64))
    mids = (lv[:-1] + lv[1:]) / 2
    flat = s.reshape(-1)
    n = flat.size
    k = max(n // 12, 6)
    idx = rng.permutation(n)
    flat[idx[:k]] = rng.choice(mids, k) + 1j * rng.choice(lv, k)
    flat[idx[k:2 * k]] = rng.choice(lv, k) + 1j * rng.choice(mids, k)
    flat[idx[2 * k:3 * k]] = rng.choice(mids, k) + 1j * rng.choice(mids, k)
    flat[idx[3 * k:4 * k]] = rng.choice(np.array([np.nan, np.inf, -np.inf + 1j, 1 - np.inf * 1j, 1e30 + 1e30j,
                                                  -1e30 + 0.5j]), k)
    return s


def _plane_rows(planes, N, B):
    """[B, 6N] int32 bit patterns: row r is lane r % 64 of tile r / 64, the tile being
    [N][64] float4 then [N][64] float2 (include/tdec.h)."""
    tiles = (B + 63) // 64
    P = planes[:tiles * N * 384].view(tiles, N * 384)
    X = P[:, :N * 256].view(tiles, N, 64, 4).permute(0, 2, 1, 3).reshape(tiles * 64, N * 4)
    Z = P[:, N * 256:].view(tiles, N, 64, 2).permute(0, 2, 1, 3).reshape(tiles * 64, N * 2)
    return torch.cat([X, Z], dim=1)[:B].contiguous().view(torch.int32)


def _entry_symbols(c, bps, S):
    """The symbol that feeds each entry of a _plane_rows row (int64 [6N]; -1: punctured, or
    past the S * bps LLRs the symbols give: the entry is 0.0 whatever the noise variance):
    the de-puncture walk over the LLR indices."""
    n_llr = c.handle.llr_len
    walk = O.depuncture(np.arange(1, n_llr + 1, dtype=np.float32), c.N, c.punct["period"], T.puncture_matrix(c.punct))
    idx = walk.astype(np.int64) - 1                                 # [6][N] LLR index, -1: punctured
    ent = np.concatenate([idx[:4].T.reshape(-1), idx[4:].T.reshape(-1)])
    return np.where((ent >= 0) & (ent < S * bps), ent // bps, -1)


def _check_planes(c, syms, mod, nv, div_f32, algo, cons=None, vals=None):
    cons = D.constellation(mod) if cons is None else cons
    bps = D.MODULATIONS[mod]["bps"]
    B = syms.shape[0]
    c.reserve(B)
    ds = torch.from_numpy(syms).cuda()
    n = c.planes_bytes(B) // 4
    got_p = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    dnv = torch.from_numpy(nv).cuda()
    c.demap_planes_device(ds, cons, bps, dnv, got_p, div_f32=div_f32, algo=algo)
    got = _plane_rows(got_p, c.N, B)
    ent = torch.from_numpy(_entry_symbols(c, bps, syms.shape[1])).cuda()
    ent_nv = dnv[:, ent.clamp(min=0)]                               # [B, 6N]: the value behind each entry
    ref_p = torch.empty_like(got_p)
    seen = torch.zeros_like(got, dtype=torch.bool)
    for v in vals:
        c.demap_planes_device(ds, cons, bps, float(v), ref_p, div_f32=div_f32, algo=algo)
        ref = _plane_rows(ref_p, c.N, B)
        mask = (torch.isnan(ent_nv) if np.isnan(v) else ent_nv == v) | (ent < 0)
        assert mask.any() and torch.equal(got[mask], ref[mask]), f"nv = {v}"
        seen |= mask
    assert bool(seen.all())
    return got


def _syms_for(c, mod, rng, B, maker=_noisy):
    bps = D.MODULATIONS[mod]["bps"]
    return maker(D.constellation(mod), rng, (B, -(-c.n_coded // bps)))


# ---- the plane kernels ----------------------------------------------------------------------
@pytest.mark.parametrize("n,rate", [(48, "1/3"), (48, "1/2")])
@pytest.mark.parametrize("div_f32", [0, 1])
@pytest.mark.parametrize("mod", MODS)
def test_planes_maxlog_symbols_equal_scalar_launches(mod, div_f32, n, rate):
    c = _codec(n, rate)
    rng = np.random.default_rng(sum(map(ord, mod + rate)) + div_f32)
    syms = _syms_for(c, mod, rng, B_PLANES)
    syms[B_PLANES // 2, 1] = np.nan
    nv = _scatter(PLANE_VALS, *syms.shape, start=div_f32 + len(mod))
    _check_planes(c, syms, mod, nv, div_f32, "max-log", vals=PLANE_VALS)


@pytest.mark.parametrize("n,rate", [(48, "1/3"), (48, "1/2")])
@pytest.mark.parametrize("mod", MODS)
def test_planes_logmap_symbols_equal_scalar_launches(mod, n, rate):
    c = _codec(n, rate)
    rng = np.random.default_rng(sum(map(ord, mod + rate)))
    syms = _syms_for(c, mod, rng, B_PLANES)
    syms[B_PLANES // 2, 1] = np.inf
    _check_planes(c, syms, mod, _scatter(PLANE_VALS, *syms.shape, start=len(mod)), 0, "log-map", vals=PLANE_VALS)


@pytest.mark.parametrize("algo,div_f32", [("max-log", 0), ("max-log", 1), ("log-map", 0)])
def test_planes_padded_walk(algo, div_f32):
    """N = 212 at 16QAM rate 2/3: the puncture period does not divide N, so the decoder's
    walk is longer than the symbols' LLRs (its tail is zero-padded) and the last symbol is
    only partly coded bits."""
    c = _codec(212, "2/3")
    assert c.handle.llr_len > -(-c.n_coded // 4) * 4 > c.n_coded
    rng = np.random.default_rng(212 + div_f32)
    syms = _syms_for(c, "16QAM", rng, B_PLANES)
    _check_planes(c, syms, "16QAM", _scatter(PLANE_VALS, *syms.shape, start=div_f32), div_f32, algo, vals=PLANE_VALS)


# ---- the decline path of the split kernels ----------------------------------------------------
@pytest.mark.parametrize("div_f32,f64_table", [(0, False), (1, False), (0, True)])
@pytest.mark.parametrize("mod", ["16QAM", "64QAM", "256QAM"])
def test_split_declined_symbols_take_their_own_value(mod, div_f32, f64_table):
    """Symbols the fast search declines (boundaries, NaN, +-inf, 1e30) among symbols of
    differing nv, +inf and NaN included: they go through k_demap_fix with their own value."""
    c = _codec(48, "1/3")
    cons = D.constellation(mod)
    rng = np.random.default_rng(sum(map(ord, mod)) + div_f32)
    syms = _syms_for(c, mod, rng, 130, maker=_boundary)
    _check_planes(c, syms, mod, _scatter(DECLINE_VALS, *syms.shape), div_f32, "max-log",
                  cons.astype(np.complex128) if f64_table else cons, vals=DECLINE_VALS)


def test_split_overflowing_declines_redo_their_tiles_per_symbol():
    """The shape of test_gpu_demap_split.py::test_split_overflowing_declines_redo_their_tiles
    (64QAM, 8 192 codewords x 752 symbols, 90 % NaN: the declines overflow the list and
    whole tiles are redone) with two nv values alternating symbol by symbol."""
    rng = np.random.default_rng(77)
    mod = "64QAM"
    c = _codec(752, "1/3")
    cons = D.constellation(mod)
    B, S = 8192, -(-c.n_coded // 6)
    syms = (cons[rng.integers(0, 64, (B, S))] + 0.1 * (rng.standard_normal((B, S)) +
                                                        1j * rng.standard_normal((B, S)))).astype(np.complex64)
    syms[rng.random((B, S)) < 0.9] = np.nan
    nv = np.where((np.arange(B)[:, None] + np.arange(S)[None, :]) % 2 == 0, 0.05, 0.3)
    _check_planes(c, syms, mod, nv, 0, "max-log", vals=[0.05, 0.3])


# ---- the flat kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["max-log", "log-map"])
@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("mod", MODS)
def test_flat_symbols_equal_scalar_calls_and_the_oracle(mod, dtype, sign, algo):
    """compute_llr_device([B, S], nv [B, S]) against the scalar launch (tdec_demap_dev /
    tdec_demap_logmap_dev itself, with the division dtype the tensor path is defined to
    take) over the whole batch per distinct value, f64 bit patterns by symbol; max-log
    also against oracle.demap per value.  One value is below the floor, one NaN, one
    +inf.  5 x 37 symbols: rows do not align with blocks."""
    B, S = 5, 37
    case = MODS.index(mod) * 8 + (dtype == np.complex128) * 4 + (sign < 0) * 2 + (algo == "log-map")
    nv = _scatter(FLAT_VALS, B, S, start=case)
    rng = np.random.default_rng(case)
    cons = D.constellation(mod)
    syms = _noisy(cons, rng, (B, S)).astype(dtype)
    syms[3, 7] = np.nan
    ds = torch.from_numpy(syms).cuda()
    bps = D.MODULATIONS[mod]["bps"]
    got = D.compute_llr_device(ds, mod, torch.from_numpy(nv).cuda(), sign=sign, algo=algo)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, S * bps)
    got = got.cpu().numpy().reshape(B, S, bps)
    f64, div_f32, _ = D.demap_mode(dtype, cons.dtype, np.float64(1.0))
    tab = np.ascontiguousarray(cons.astype(np.complex128 if f64 else np.complex64))
    st = torch.cuda.current_stream().cuda_stream
    seen = 0
    for v in FLAT_VALS:
        ref = torch.empty(B * S * bps, dtype=torch.float64, device="cuda")
        args = (0, N.ptr(ds), int(dtype == np.complex128), B * S, N.ptr(tab), int(f64), len(tab), bps, float(v))
        if algo == "log-map":
            N.check(N.lib().tdec_demap_logmap_dev(*args, sign, N.ptr(ref), st))
        else:
            N.check(N.lib().tdec_demap_dev(*args, int(div_f32), sign, N.ptr(ref), st))
        ref = ref.cpu().numpy().reshape(B, S, bps)
        m = _is(nv, v)
        assert m.any() and np.array_equal(got[m].view(np.int64), ref[m].view(np.int64)), f"nv = {v}"
        if algo == "max-log":
            orc = sign * O.demap(syms[m], cons, bps, v, div_f32).reshape(-1, bps)
            np.testing.assert_array_equal(got[m], orc, err_msg=f"oracle, nv = {v}")
        seen += int(m.sum())
    assert seen == B * S
    assert np.isnan(got[3, 7]).all() and np.isnan(got[_is(nv, np.nan)]).all()
    if algo == "max-log":
        fin = _is(nv, np.inf) & np.isfinite(syms)
        assert fin.any() and not got[fin].any()                      # +inf: an erasure, zero LLRs


# ---- the equaliser ------------------------------------------------------------------------
def _bits_equal(a, b):
    """IEEE ==, NaN at the same positions, and the same zeros' signs."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype in (np.float32, np.complex64) else np.uint64
    na, nb = np.isnan(a.view(a.real.dtype)), np.isnan(b.view(b.real.dtype))
    return np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


@pytest.mark.parametrize("rows_nv", [False, True])
@pytest.mark.parametrize("B,S,coh", [(69, 72, 1), (3, 301, 7), (1, 1, 1), (5, 4512, 4512)])
def test_equaliser_equals_its_numpy_restatement(B, S, coh, rows_nv):
    rng = np.random.default_rng(B * S + coh + rows_nv)
    nh = -(-S // coh)
    cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)  # noqa: E731
    y = (cn(B, S) * np.float32(10) ** rng.integers(-3, 4, (B, S))).astype(np.complex64)
    h = (cn(B, nh) * np.float32(10) ** rng.integers(-2, 3, (B, nh))).astype(np.complex64)
    special_h = np.array([0, 1e-42 + 3e-43j, np.nan + 1j, 1 + np.inf * 1j, -np.inf, 1e25 - 1e25j, 1e-30j], np.complex64)
    special_y = np.array([np.nan, np.inf + 1j, 1 - np.inf * 1j, 0, 1e38 + 1e38j, 1e-44], np.complex64)
    hf, yf = h.reshape(-1), y.reshape(-1)
    hi = rng.permutation(hf.size)[:len(special_h)]
    hf[hi] = special_h[:len(hi)]
    yi = rng.permutation(yf.size)[:len(special_y)]
    yf[yi] = special_y[:len(yi)]
    nv = (10.0 ** rng.uniform(-3, 1, B)) if rows_nv else 0.0371
    dy, dh = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
    z, nvs = D.equalize_device(dy, dh, torch.from_numpy(nv).cuda() if rows_nv else nv, coh=coh)
    assert z.dtype == torch.complex64 and tuple(z.shape) == (B, S)
    assert nvs.dtype == torch.float64 and tuple(nvs.shape) == (B, S)
    rz, rnv = F.equalize(y, h, nv, coh)
    assert _bits_equal(z.cpu().numpy(), rz)
    assert _bits_equal(nvs.cpu().numpy(), rnv)
    r0, j0 = divmod(int(hi[0]), nh)                                  # the zero gain's symbols are erasures
    assert not z[r0, j0 * coh:(j0 + 1) * coh].cpu().numpy().any()
    assert np.isposinf(nvs[r0, j0 * coh:(j0 + 1) * coh].cpu().numpy()).all()
    # out= buffers, and a misaligned y (a view one symbol into a buffer): the 8-byte path
    if B * S > 1:
        buf = torch.zeros(B * S + 1, dtype=torch.complex64, device="cuda")
        buf[1:] = dy.reshape(-1)
        oz, onv = torch.empty_like(dy), torch.empty((B, S), dtype=torch.float64, device="cuda")
        r = D.equalize_device(buf[1:].view(B, S), dh, torch.from_numpy(nv).cuda() if rows_nv else nv, coh=coh,
                              out=oz, nv_out=onv)
        assert r[0] is oz and r[1] is onv
        assert _bits_equal(oz.cpu().numpy(), rz) and _bits_equal(onv.cpu().numpy(), rnv)


# ---- the generator ------------------------------------------------------------------------
@pytest.mark.parametrize("K,coh", [(0.0, 1), (4.0, 5)])
def test_fading_generator_streams_and_split_invariance(K, coh):
    c = _codec(752, "1/3")
    seed, B, mod = 4242, 1000, "16QAM"
    fading = {"K": K, "coh": coh}
    info, full, n0, h = W.make_symbols(c, B, mod, 2.0, seed, "cuda", cw0=0, fading=fading)
    S = full.shape[1]
    assert tuple(h.shape) == (B, -(-S // coh)) and h.dtype == torch.complex64
    # a 400 + 600 split equals one batch of 1000 exactly, gains included
    a = W.make_symbols(c, 400, mod, 2.0, seed, "cuda", cw0=0, want_info=False, fading=fading)
    b = W.make_symbols(c, 600, mod, 2.0, seed, "cuda", cw0=400, want_info=False, fading=fading)
    assert torch.equal(torch.cat([a[1], b[1]]), full) and torch.equal(torch.cat([a[3], b[3]]), h)
    # the AWGN entry's info bits and noise
    info0, awgn, n00 = W.make_symbols(c, 64, mod, 2.0, seed, "cuda", cw0=0)
    assert n00 == n0 and torch.equal(info0, info[:64])
    clean = W.make_symbols(c, 64, mod, 1000.0, seed, "cuda", cw0=0, want_info=False)[1].cpu().numpy()
    awgn_noise = awgn.cpu().numpy().astype(np.complex128) - clean
    hs = h[:64].cpu().numpy().astype(np.complex128)[:, np.arange(S) // coh]
    noise = full[:64].cpu().numpy().astype(np.complex128) - hs * clean
    print("max |fading noise - awgn noise|", np.max(np.abs(noise - awgn_noise)))
    assert np.max(np.abs(noise - awgn_noise)) < 2e-5
    assert np.max(np.abs(awgn_noise - WR.awgn(np.arange(64), S, seed, np.sqrt(n0 / 2)))) < 2e-5
    # the gains against their restatement
    ref = F.gains(np.arange(B), h.shape[1], seed, K)
    print("max |gain - restatement|", np.max(np.abs(h.cpu().numpy() - ref)))
    assert np.max(np.abs(h.cpu().numpy() - ref)) < 2e-5


# ---- equalise -> demap -> decode on one stream --------------------------------------------
@pytest.fixture(scope="module")
def chain_ref():
    """Per coh: the symbols, gains and N0 of 130 N = 212, r = 1/2 QPSK codewords over a
    Rayleigh channel at 6 dB, and the reference chain's LLRs (the restated equaliser, then
    oracle.demap per symbol), computed once."""
    c = _codec(212, "1/2", interleaver="valid-perm")
    out = {}
    for coh in (1, 16):
        _, syms, n0, h = W.make_symbols(c, 130, "QPSK", 6.0, 99, "cuda", want_info=False, fading={"K": 0.0, "coh": coh})
        z, nvs = F.equalize(syms.cpu().numpy(), h.cpu().numpy(), n0, coh)
        cons = D.constellation("QPSK")
        _, div_f32, _ = D.demap_mode(np.complex64, cons.dtype, np.float64(1.0))
        llr = -F.demap_per_symbol(z, cons, 2, nvs, div_f32)          # decoder sign
        out[coh] = (syms, h, n0, llr[:, :c.n_coded].astype(np.float32))
    return out


@pytest.mark.parametrize("coh", [1, 16])
def test_chain_equals_the_reference_chain(chain_ref, coh):
    c = _codec(212, "1/2", interleaver="valid-perm")
    syms, h, n0, llr = chain_ref[coh]
    t, _ = O.trellis()
    want = O.decode_batch(llr, c.N, c.punct["period"], T.puncture_matrix(c.punct), c.iterations, c.perm, c.inv_perm, t)
    dev = torch.device("cuda", 0)
    pipe = W.DevicePipeline(c, "QPSK", 130, dev, csi=True)
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        bits = pipe.run(syms, n0, stream=st, csi=h, coh=coh).clone()
    st.synchronize()
    assert np.array_equal(bits.cpu().numpy(), want)
    # a [B] noise variance tensor in front of the equaliser: the same bits
    nv = torch.full((130,), float(n0), dtype=torch.float64, device=dev)
    assert torch.equal(pipe.run(syms, nv, csi=h, coh=coh), bits)


def test_chain_early_stop_tile(chain_ref):
    """The same symbols through the early-stop tile decoder: the bits and iteration counts
    of the restated rule (tests/early_stop_ref.py) on the reference chain's LLRs."""
    c = _codec(212, "1/2", interleaver="valid-perm", early_stop=True, es_decoder="tile")
    syms, h, n0, llr = chain_ref[16]
    t, _ = O.trellis()
    want_bits, _, want_iters = ES.decode_early_stop_batch(llr, c.N, c.punct, c.iterations, c.perm, c.inv_perm, t)
    pipe = W.DevicePipeline(c, "QPSK", 130, torch.device("cuda", 0), csi=True)
    bits = pipe.run(syms, n0, csi=h, coh=16)
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    assert np.array_equal(pipe.n_iter[:130].cpu().numpy(), want_iters)


# ---- argument conventions of the new calls (include/tdec.h) ---------------------------------
def test_new_calls_refuse_bad_arguments_and_accept_empty_batches():
    c = _codec(48, "1/3")
    L, EINVAL = N.lib(), N.TDEC_EINVAL
    B, S = 3, 36
    tab = np.ascontiguousarray(D.constellation("16QAM").astype(np.complex64))
    syms = torch.zeros((B, S), dtype=torch.complex64, device="cuda")
    nv = torch.full((B, S), 0.1, dtype=torch.float64, device="cuda")
    llr = torch.full((B * S * 4,), np.nan, dtype=torch.float64, device="cuda")
    planes = torch.full((c.planes_bytes(B) // 4,), np.nan, dtype=torch.float32, device="cuda")
    p = N.ptr
    for name, div in (("tdec_symnv_demap_dev", [1]), ("tdec_symnv_demap_logmap_dev", [])):
        f = getattr(L, name)
        assert f(0, p(syms), 0, B, S, p(tab), 0, 16, 4, None, *div, -1, p(llr), None) == EINVAL
        assert f(0, None, 0, B, S, p(tab), 0, 16, 4, p(nv), *div, -1, p(llr), None) == EINVAL
        assert f(0, p(syms), 0, -1, S, p(tab), 0, 16, 4, p(nv), *div, -1, p(llr), None) == EINVAL
        assert f(0, p(syms), 0, B, S, p(tab), 0, 16, 9, p(nv), *div, -1, p(llr), None) == EINVAL
        assert f(0, p(syms), 0, 0, S, p(tab), 0, 16, 4, p(nv), *div, -1, p(llr), None) == 0
    for name, div in (("tdec_symnv_demap_planes_dev", [1]), ("tdec_symnv_demap_planes_logmap_dev", [])):
        f = getattr(L, name)
        h = c.handle.h
        assert f(h, B, p(syms), S, p(tab), 0, 16, 4, None, *div, p(planes), None) == EINVAL
        assert f(None, B, p(syms), S, p(tab), 0, 16, 4, p(nv), *div, p(planes), None) == EINVAL
        assert f(h, B, p(syms), 0, p(tab), 0, 16, 4, p(nv), *div, p(planes), None) == EINVAL
        assert f(h, -1, p(syms), S, p(tab), 0, 16, 4, p(nv), *div, p(planes), None) == EINVAL
        assert f(h, 0, None, S, p(tab), 0, 16, 4, None, *div, None, None) == 0
    z = torch.full((B, S), np.nan, dtype=torch.complex64, device="cuda")
    eq = L.tdec_equalize_dev
    assert eq(0, p(syms), p(syms), B, S, 0, 0.1, None, p(z), p(nv), None) == EINVAL      # coh < 1
    assert eq(0, None, p(syms), B, S, 1, 0.1, None, p(z), p(nv), None) == EINVAL
    assert eq(0, p(syms), None, B, S, 1, 0.1, None, p(z), p(nv), None) == EINVAL
    assert eq(0, p(syms), p(syms), B, S, 1, 0.1, None, None, p(nv), None) == EINVAL
    assert eq(0, p(syms), p(syms), -1, S, 1, 0.1, None, p(z), p(nv), None) == EINVAL
    assert eq(0, None, None, 0, S, 1, 0.1, None, None, None, None) == 0
    wf = L.tdec_workload_fading_dev
    t32 = tab.view(np.float32)
    hh = torch.empty((B, S), dtype=torch.complex64, device="cuda")
    Sw = -(-c.handle.enc_len // 4)
    y = torch.full((B, Sw), np.nan, dtype=torch.complex64, device="cuda")
    for k, coh, gains in ((-1.0, 1, hh), (np.inf, 1, hh), (np.nan, 1, hh), (0.0, 0, hh), (0.0, 1, None)):
        assert wf(c.handle.h, B, 0, 1, p(t32), 16, 4, 0.1, k, coh, p(y), p(gains), None, None) == EINVAL
    assert wf(c.handle.h, 0, 0, 1, p(t32), 16, 4, 0.1, 0.0, 1, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(llr).all()) and bool(torch.isnan(planes).all())             # nothing was written
    assert bool(torch.isnan(z.real).all()) and bool(torch.isnan(y.real).all())
    with pytest.raises(ValueError):
        W.make_symbols(c, B, "16QAM", 2.0, 1, "cuda", fading={"K": 0.0, "coh": 1, "doppler": 3})


# ---- ABI argument errors of the fading generator (tests/generator_abi.py) ----
@pytest.mark.parametrize("call,case", GA.params("tdec_workload_fading_dev"))
def test_generator_abi_refusals(call, case):
    GA.check(call, case)
