"""Per-row noise variance on the device.

The contract is exact: row r of a per-row launch is, bit for bit, row r of the
existing scalar launch called with noise_var = nv[r].  So every demapper test here
runs the scalar entry point on the whole batch once per distinct value of the
vector, takes the rows that carry that value, and compares bit patterns (NaNs at
the same positions included).  The vector mixes, lane by lane, a value below the
0.005 floor, the floor, ordinary values, values above the unscaled division's
range (2^16), inf and NaN.  The estimator is compared with its numpy restatement
(tests/noise_var_ref.py) at rtol 1e-11: all terms are non-negative, S <= 4512, and
f64 sums of them in any order differ by about S * 2^-53 relative."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import noise_var_ref as R  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

MODS = ["BPSK", "QPSK", "8PSK", "16QAM", "64QAM", "256QAM"]
VALS = [0.001, 0.005, 0.05, 0.3, 7.0, 1e5, 1e300, np.inf, np.nan]
BATCHES = [1, 67, 130]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _nv_vector(B, start=0):
    """The values of VALS in turn (from `start`), shuffled with a fixed seed so that
    neighbouring lanes of a tile differ."""
    v = np.array(VALS)[(np.arange(B) + start) % len(VALS)]
    return np.random.default_rng(1234 + B).permutation(v)


def _rows_with(nv, v):
    return np.flatnonzero(np.isnan(nv) if np.isnan(v) else nv == v)


def _distinct(nv):
    return [v for v in VALS if len(_rows_with(nv, v))]


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
    tables' fast search declines and k_demap_fix redoes with the row's value."""
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


def _check_planes(c, syms, mod, nv, div_f32, algo, cons=None):
    cons = D.constellation(mod) if cons is None else cons
    bps = D.MODULATIONS[mod]["bps"]
    B = syms.shape[0]
    c.reserve(B)
    ds = torch.from_numpy(syms).cuda()
    n = c.planes_bytes(B) // 4
    got_p = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    c.demap_planes_device(ds, cons, bps, torch.from_numpy(nv).cuda(), got_p, div_f32=div_f32, algo=algo)
    got = _plane_rows(got_p, c.N, B)
    ref_p = torch.empty_like(got_p)
    seen = 0
    for v in _distinct(nv):
        c.demap_planes_device(ds, cons, bps, float(v), ref_p, div_f32=div_f32, algo=algo)
        rows = torch.from_numpy(_rows_with(nv, v)).cuda()
        ref = _plane_rows(ref_p, c.N, B)
        assert torch.equal(got[rows], ref[rows]), f"nv = {v}"
        seen += len(rows)
    assert seen == B
    return got_p


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("rate", ["1/3", "1/2"])
@pytest.mark.parametrize("div_f32", [0, 1])
@pytest.mark.parametrize("mod", MODS)
def test_planes_maxlog_rows_equal_scalar_launches(mod, div_f32, rate, B):
    c = _codec(48, rate)
    bps = D.MODULATIONS[mod]["bps"]
    rng = np.random.default_rng(sum(map(ord, mod + rate)) + B + div_f32)
    syms = _noisy(D.constellation(mod), rng, (B, -(-c.n_coded // bps)))
    syms[B // 2, 1] = np.nan
    _check_planes(c, syms, mod, _nv_vector(B, start=div_f32 + len(rate + mod)), div_f32, "max-log")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod", MODS)
def test_planes_logmap_rows_equal_scalar_launches(mod, B):
    c = _codec(48, "1/3")
    bps = D.MODULATIONS[mod]["bps"]
    rng = np.random.default_rng(sum(map(ord, mod)) + B)
    syms = _noisy(D.constellation(mod), rng, (B, -(-c.n_coded // bps)))
    syms[B // 2, 1] = np.inf
    _check_planes(c, syms, mod, _nv_vector(B, start=len(mod)), 0, "log-map")


@pytest.mark.parametrize("div_f32,f64_table", [(0, False), (1, False), (0, True)])
@pytest.mark.parametrize("mod", ["16QAM", "64QAM", "256QAM"])
def test_split_declined_symbols_take_their_rows_value(mod, div_f32, f64_table):
    """Symbols the fast search declines (boundaries, NaN, +-inf, 1e30), in rows of
    differing nv: they go through k_demap_fix with the row's value."""
    c = _codec(48, "1/3")
    bps = D.MODULATIONS[mod]["bps"]
    cons = D.constellation(mod)
    rng = np.random.default_rng(sum(map(ord, mod)) + div_f32)
    syms = _boundary(cons, rng, (130, -(-c.n_coded // bps)))
    _check_planes(c, syms, mod, _nv_vector(130), div_f32, "max-log", cons.astype(np.complex128) if f64_table else cons)


def test_split_overflowing_declines_redo_their_tiles_per_row():
    """The shape of test_gpu_demap_split.py::test_split_overflowing_declines_redo_their_tiles
    (64QAM, 8 192 codewords x 752 symbols, 90 % NaN: the declines overflow the list and
    whole tiles are redone) with two nv values alternating lane by lane."""
    rng = np.random.default_rng(77)
    mod = "64QAM"
    c = _codec(752, "1/3")
    cons = D.constellation(mod)
    B, S = 8192, -(-c.n_coded // 6)
    syms = (cons[rng.integers(0, 64, (B, S))] + 0.1 * (rng.standard_normal((B, S)) +
                                                        1j * rng.standard_normal((B, S)))).astype(np.complex64)
    syms[rng.random((B, S)) < 0.9] = np.nan
    nv = np.where(np.arange(B) % 2 == 0, 0.05, 0.3)
    c.reserve(B)
    ds = torch.from_numpy(syms).cuda()
    got_p = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
    c.demap_planes_device(ds, cons, 6, torch.from_numpy(nv).cuda(), got_p)
    got = _plane_rows(got_p, c.N, B)
    ref_p = torch.empty_like(got_p)
    for k, v in enumerate((0.05, 0.3)):
        c.demap_planes_device(ds, cons, 6, v, ref_p)
        assert torch.equal(got[k::2], _plane_rows(ref_p, c.N, B)[k::2]), f"nv = {v}"


@pytest.mark.parametrize("algo", ["max-log", "log-map"])
@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("mod", MODS)
def test_flat_rows_equal_scalar_calls(mod, dtype, sign, algo):
    """compute_llr_device([B, S], nv tensor) against the scalar launch row by row, f64 bit
    patterns.  The scalar launch is tdec_demap_dev / tdec_demap_logmap_dev itself with
    noise_var = nv[r] and the division dtype the tensor path is defined to take (that of
    a numpy float64 scalar): compute_llr_device's own scalar form would switch a value
    below the floor to the f32 division (numpy's max(nv, 0.005) hands back the Python
    float), which is a rule about Python scalars, not about the launch.  5 x 37 symbols:
    rows do not align with blocks."""
    B, S = 5, 37
    case = MODS.index(mod) * 8 + (dtype == np.complex128) * 4 + (sign < 0) * 2 + (algo == "log-map")
    nv = _nv_vector(B, start=case)     # 5 of the 9 values, rotating with the case: all are met
    rng = np.random.default_rng(case)
    syms = _noisy(D.constellation(mod), rng, (B, S)).astype(dtype)
    syms[3, 7] = np.nan
    ds = torch.from_numpy(syms).cuda()
    bps = D.MODULATIONS[mod]["bps"]
    got = D.compute_llr_device(ds, mod, torch.from_numpy(nv).cuda(), sign=sign, algo=algo)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, S * bps)
    cons = D.constellation(mod)
    f64, div_f32, _ = D.demap_mode(dtype, cons.dtype, np.float64(1.0))
    tab = np.ascontiguousarray(cons.astype(np.complex128 if f64 else np.complex64))
    st = torch.cuda.current_stream().cuda_stream
    for r in range(B):
        ref = torch.empty(S * bps, dtype=torch.float64, device="cuda")
        args = (0, N.ptr(ds[r]), int(dtype == np.complex128), S, N.ptr(tab), int(f64), len(tab), bps, float(nv[r]))
        if algo == "log-map":
            N.check(N.lib().tdec_demap_logmap_dev(*args, sign, N.ptr(ref), st))
        else:
            N.check(N.lib().tdec_demap_dev(*args, int(div_f32), sign, N.ptr(ref), st))
        assert torch.equal(got[r].view(torch.int64), ref.view(torch.int64)), f"row {r}, nv = {nv[r]}"
    assert bool(torch.isnan(got[3, 7 * bps:(7 + 1) * bps]).all())


def test_every_value_is_met_by_the_flat_cases():
    met = set()
    for case in range(len(MODS) * 8):
        met |= {repr(float(v)) for v in _nv_vector(5, start=case)}
    assert met == {repr(float(v)) for v in VALS}


# ---- the estimator --------------------------------------------------------------------
def _estimator_rows(mod, B, S):
    cons = D.constellation(mod)
    rng = np.random.default_rng(sum(map(ord, mod)) + S)
    sigma = 10 ** rng.uniform(-2.0, -0.3, (B, 1))          # a different SNR per row
    syms = (cons[rng.integers(0, len(cons), (B, S))] +
            sigma * (rng.standard_normal((B, S)) + 1j * rng.standard_normal((B, S)))).astype(np.complex64)
    syms[0] = cons[rng.integers(0, len(cons), S)].astype(np.complex64)     # below the floor
    if B > 2:
        syms[2, S // 2] = np.nan
    if B > 5:
        syms[5, S - 1] = np.inf + 0j
    return cons, syms


@pytest.mark.parametrize("mod,B,S", [("16QAM", 130, 72), ("QPSK", 67, 144), ("256QAM", 7, 4512), ("8PSK", 130, 301),
                                     ("BPSK", 3, 1), ("64QAM", 67, 257)])
def test_estimator_equals_its_numpy_restatement(mod, B, S):
    cons, syms = _estimator_rows(mod, B, S)
    ds = torch.from_numpy(syms).cuda()
    got_t = D.estimate_noise_var_device(ds, mod)
    assert got_t.dtype == torch.float64 and tuple(got_t.shape) == (B,) and got_t.device == ds.device
    got = got_t.cpu().numpy()
    ref = R.noise_var_rows(syms, cons, 0.02)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    fin = ~np.isnan(ref)
    print(mod, B, S, "max rel diff", np.max(np.abs(got[fin] - ref[fin]) / ref[fin]))
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-11, atol=0)
    assert got[0] == 0.02                                   # a row below the floor: exactly the floor
    if B > 2:
        assert np.isnan(got[2])                             # one NaN symbol
    if B > 5:
        assert np.isnan(got[5])                             # one infinite symbol
    # another floor, and an out= buffer
    out = torch.empty(B, dtype=torch.float64, device="cuda")
    assert D.estimate_noise_var_device(ds, mod, floor=0.5, out=out) is out
    ref5 = R.noise_var_rows(syms, cons, 0.5)
    fin5 = ~np.isnan(ref5)
    np.testing.assert_allclose(out.cpu().numpy()[fin5], ref5[fin5], rtol=1e-11, atol=0)
    # a row's value does not depend on the batch: bit patterns at B = 1
    for r in sorted({0, 1, B // 2, B - 1}):
        one = D.estimate_noise_var_device(ds[r:r + 1].contiguous(), mod)
        assert torch.equal(one.view(torch.int64), got_t[r:r + 1].view(torch.int64)), r


# ---- estimate -> demap -> decode on one stream ------------------------------------------
@pytest.mark.parametrize("variant", ["max-log", "log-map", "early-stop-tile"])
def test_chain_equals_row_wise_scalar_runs(variant):
    """Two groups of N = 48, r = 1/3, 16QAM codewords at 2 dB and 8 dB, interleaved row
    by row: estimate -> DevicePipeline.run(syms, nv tensor) queued on one stream gives
    the bits of row-wise scalar runs with each row's estimate read back."""
    mod, B = "16QAM", 130
    kw = dict(early_stop=True, es_decoder="tile") if variant == "early-stop-tile" else {}
    c = _codec(48, "1/3", **kw)
    dev = torch.device("cuda", 0)
    _, lo, _ = W.make_symbols(c, B // 2, mod, 2.0, 11, dev, want_info=False)
    _, hi, _ = W.make_symbols(c, B // 2, mod, 8.0, 12, dev, want_info=False)
    syms = torch.stack([lo, hi], dim=1).reshape(B, -1).contiguous()
    pipe = W.DevicePipeline(c, mod, B, dev, demap="log-map" if variant == "log-map" else "max-log")
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        nv = D.estimate_noise_var_device(syms, mod, stream=st)
        bits = pipe.run(syms, nv, stream=st).clone()
    st.synchronize()
    nv_h = nv.cpu().numpy()
    assert nv_h[0::2].mean() > nv_h[1::2].mean() and (nv_h >= 0.02).all()   # the two groups differ
    for r in range(B):
        ref = pipe.run(syms[r:r + 1], np.float64(nv_h[r]))
        assert torch.equal(ref[0], bits[r]), r
