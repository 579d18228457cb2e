"""Every kernel that writes the decoder's planes, on every codec and modulation.

tests/test_gpu_codec_matrix.py pins the kernels that read the planes on all 28 codecs;
this module pins the ones that write them.  Their index arithmetic -- an item's chunk of
dm_kc(bps) couples and its ragged last chunk, the symbols that straddle a chunk boundary
and their LDS column, the surplus bits of the last symbol, the zero tail where n_coded is
shorter than the walk, k_demap_fix's dst table, the thread-to-item mapping by ns -- all
depends on (N, rate, bits per symbol), so every test runs on the 168 cases of
tests/plane_matrix.py (28 codecs x BPSK, QPSK, 8PSK, 16QAM, 64QAM, 256QAM), 69 rows each
(one full 64-lane tile and a partial one), on symbols whose ties and non-finite values
the split search declines:

  test_maxlog_scalar        k_demap_planes (plain, and split with k_demap_fix) against
                            the host chain (oracle.demap, negated)
  test_logmap_scalar        k_demap_planes_lm against the flat log-MAP kernel, which
                            tests/test_gpu_demap_logmap.py holds to the float64 definition
  test_tensor_noise_var     RowNv<1> (float64 [69]) and RowNv<2> (float64 [69, S]) of
                            both, three values assigned cyclically over the rows / over
                            the flattened symbols; max-log against one oracle.demap per
                            value, log-MAP against the flat kernel with the same tensor
  test_fused                k_demap_decode / DemapPro wherever fused_available says so,
                            for the max-log and the log-MAP codec: bits and L_final of
                            decode_planes_device on test_maxlog_scalar's plane buffer
  test_depuncture           k_depuncture and its int8 / float16 forms on the 28 codecs,
                            rows with a stride longer than the walk behind one leading
                            element, NaN (or -128) in between

The expected planes are built on the CPU from the restated de-puncture walk
(plane_matrix.reference_planes, pinned to the oracle's de-puncture at every (N, rate) by
tests/test_plane_matrix_host.py), not by k_depuncture.  Every comparison covers the whole
plane buffer and 64 guard floats behind it, which must keep their sentinel bit for bit;
planes are compared with np.testing.assert_array_equal (NaN == NaN).  There is no
tolerance anywhere in this module.  The division's dtype and the effective noise variance
are what demap.demap_mode gives for complex64 symbols and the table's dtype; the other
arithmetic variants are test_gpu_demap_split.py's.

Fused combinations available in this build, as seen on an MI355X: 112 of the 336 (codec,
algorithm, modulation) -- all 28 codecs for QPSK, 16QAM and 256QAM under the max-log
codec and for 8PSK under the log-MAP one (FUSED_AVAILABLE).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import codec_matrix as CM  # noqa: E402
import llrq_ref as Q  # noqa: E402
import plane_matrix as PM  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402

B = PM.ROWS
GUARD = 64
SENTINEL = np.float32(12345.678)   # no LLR (|llr| <= 30), no int8 multiple of a step, no float16 value
NV = 0.04
NV3 = (0.04, 0.11, 0.3)            # above the 0.005 floor and inside the unscaled divisions' range
CODEC_IDS = [CM.codec_id(*c) for c in CM.CODECS]
# (codec, algorithm, modulation) combinations with a fused kernel, as seen on an MI355X
# (a fact of the build, tdec_demap_api.hip fused_kernel; asserted by test_fused_combinations)
FUSED_AVAILABLE = 112


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_CODECS = {}


def _codec(n, rate, algo="max-log"):
    key = (n, rate, algo)
    if key not in _CODECS:
        c = _CODECS[key] = M.DVBRCS2_Turbo(n, rate, algo=algo)
        c.reserve(B)
    return _CODECS[key]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the fixtures are read-only)


def _planes(c):
    return torch.full((c.planes_bytes(B) // 4 + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")


def _check(c, planes, llr64, n, rate, want_nan=False):
    """The whole buffer against reference_planes(llr64), and the guard floats behind it."""
    ref = PM.reference_planes(llr64, n, T.PUNCTURE_PATTERNS[rate], B)
    assert ref.size == c.planes_bytes(B) // 4 == planes.numel() - GUARD
    assert np.count_nonzero(np.nan_to_num(ref)) > 0                  # the reference is not all zero
    torch.cuda.synchronize()
    got = planes.cpu().numpy()
    assert np.array_equal(got[ref.size:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "guard floats"
    np.testing.assert_array_equal(got[:ref.size], ref)
    if want_nan:   # a symbol the split search declined was written by k_demap_fix
        assert np.isnan(got[:ref.size]).any()


def _mode(mod, nv):
    """(table, bps, float32 division?, effective noise variance) of a scalar launch."""
    cons = D.constellation(mod)
    _, div32, nve = D.demap_mode(np.complex64, cons.dtype, np.float64(nv))
    return cons, PM.BPS[mod], div32, nve


# ---- a. max-log, scalar noise variance ---------------------------------------------------------
def _maxlog_planes(c, n, rate, mod):
    cons, bps, div32, nve = _mode(mod, NV)
    planes = _planes(c)
    c.demap_planes_device(_dev(PM.symbols(n, rate, mod)), cons, bps, nve, planes, div_f32=div32)
    return planes


@pytest.mark.parametrize("n,rate,mod", PM.CASES, ids=PM.CASE_IDS)
def test_maxlog_scalar(n, rate, mod):
    c = _codec(n, rate)
    _, _, div32, nve = _mode(mod, NV)
    planes = _maxlog_planes(c, n, rate, mod)
    _check(c, planes, PM.maxlog_llr(PM.symbols(n, rate, mod), mod, nve, div32), n, rate, want_nan=mod in PM.SPLIT_MODS)


# ---- b. log-MAP, scalar ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,rate,mod", PM.CASES, ids=PM.CASE_IDS)
def test_logmap_scalar(n, rate, mod):
    c = _codec(n, rate)
    cons, bps, _, nve = _mode(mod, NV)
    ds = _dev(PM.symbols(n, rate, mod))
    planes = _planes(c)
    c.demap_planes_device(ds, cons, bps, nve, planes, algo="log-map")
    llr = D.compute_llr_device(ds, mod, nve, sign=-1, algo="log-map")
    _check(c, planes, llr.cpu().numpy().reshape(B, -1), n, rate)


# ---- c. per-row and per-symbol noise variance -------------------------------------------------------
def _nv_tensor(form, S):
    """NV3 in turn over the rows, or over the flattened symbols: neighbouring lanes, and
    neighbouring symbols of one item, differ."""
    v = np.array(NV3, np.float64)
    return v[np.arange(B) % 3] if form == "rows" else v[np.arange(B * S) % 3].reshape(B, S)


@pytest.mark.parametrize("form", ["rows", "syms"])
@pytest.mark.parametrize("algo", ["max-log", "log-map"])
@pytest.mark.parametrize("n,rate,mod", PM.CASES, ids=PM.CASE_IDS)
def test_tensor_noise_var(n, rate, mod, algo, form):
    c = _codec(n, rate)
    syms = PM.symbols(n, rate, mod)
    S = syms.shape[1]
    cons, bps, div32, _ = _mode(mod, NV)
    nv = _nv_tensor(form, S)
    assert all((nv == v).any() for v in NV3)
    ds, dnv = _dev(syms), _dev(nv)
    planes = _planes(c)
    c.demap_planes_device(ds, cons, bps, dnv, planes, div_f32=div32, algo=algo)
    if algo == "log-map":
        llr = D.compute_llr_device(ds, mod, dnv, sign=-1, algo="log-map").cpu().numpy()
    else:
        llr = np.empty((B, S, bps))
        for v in NV3:   # one host chain per value; every row / symbol from its own value's
            _, _, d32, nve = _mode(mod, v)
            assert d32 == div32 and nve == v
            llr[nv == v] = PM.maxlog_llr(syms, mod, nve, d32).reshape(B, S, bps)[nv == v]
    _check(c, planes, llr.reshape(B, S * bps), n, rate, want_nan=algo == "max-log" and mod in PM.SPLIT_MODS)


# ---- d. fused demap + decode --------------------------------------------------------------------------
def _fused_mods(c):
    return [mod for mod in PM.MODS if c.fused_available(D.constellation(mod), PM.BPS[mod])]


@pytest.mark.parametrize("algo", CM.ALGOS)
@pytest.mark.parametrize("n,rate", CM.CODECS, ids=CODEC_IDS)
def test_fused(n, rate, algo):
    """Every modulation this (codec, algorithm) has a fused kernel for (none for some:
    test_fused_combinations counts them)."""
    c = _codec(n, rate, algo)
    for mod in _fused_mods(c):
        cons, bps, div32, nve = _mode(mod, NV)
        planes = _maxlog_planes(c, n, rate, mod)
        want_bits = torch.full((B, c.k_info), 7, dtype=torch.int32, device="cuda")
        want_lf = torch.full((B, c.k_info), 7.0, dtype=torch.float64, device="cuda")
        c.decode_planes_device(planes, B, want_bits, want_lf)
        bits = torch.full_like(want_bits, 9)
        lf = torch.full_like(want_lf, 9.0)
        c.reserve_fused(B)
        c.demap_decode_device(_dev(PM.symbols(n, rate, mod)), cons, bps, nve, bits, lfinal=lf, div_f32=div32)
        torch.cuda.synchronize()
        assert np.isin(want_bits.cpu().numpy(), (0, 1)).all(), mod
        assert torch.equal(bits, want_bits), mod
        np.testing.assert_array_equal(lf.cpu().numpy(), want_lf.cpu().numpy(), err_msg=mod)


def test_fused_combinations():
    per = {(n, rate, algo): _fused_mods(_codec(n, rate, algo)) for n, rate in CM.CODECS for algo in CM.ALGOS}
    count = sum(len(m) for m in per.values())
    by_mod = {mod: sum(mod in m for m in per.values()) for mod in PM.MODS}
    print("fused combinations available:", count, by_mod)
    assert count > 0, f"no fused combination available: {by_mod}"
    assert count == FUSED_AVAILABLE, f"{count} fused combinations available: {by_mod}"


# ---- e. the de-puncture kernels ---------------------------------------------------------------------
KINDS = [("f32", None), ("int8", np.float32(0.25)), ("int8", np.float32(0.3)), ("f16", None)]
KIND_IDS = ["f32", "int8-0.25", "int8-0.3", "f16"]


def _rows(kind, rng, L):
    if kind == "int8":
        q = rng.integers(-128, 128, (B, L)).astype(np.int8)
        q[:, -1] = rng.choice(np.int8([-128, 127, -1]), B)           # the walk's last LLR is never 0
        q.flat[:3] = np.int8([-128, 127, 0])
        return q
    x = (8 * rng.standard_normal((B, L))).astype(np.float32)
    sp = np.float32([np.inf, -np.inf, np.nan, 65504.0, -65504.0, 6e-8, -6e-8, -0.0])   # all float16 values
    at = rng.permutation(B * (L - 1))[:max(8, B * L // 16)]
    x[:, :-1].flat[at] = sp[np.arange(len(at)) % len(sp)]
    return x.astype(np.float16) if kind == "f16" else x


@pytest.mark.parametrize("kind,step", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("n,rate", CM.CODECS, ids=CODEC_IDS)
def test_depuncture(n, rate, kind, step):
    c = _codec(n, rate)
    L = CM.walk(n, rate)
    assert c.handle.llr_len == L
    rows = _rows(kind, np.random.default_rng([5, n, CM.CODECS.index((n, rate)), KINDS.index((kind, step))]), L)
    wide = Q.dequantize_i8(rows, step) if kind == "int8" else Q.dequantize_f16(rows) if kind == "f16" else rows
    assert wide.dtype == np.float32
    # stride walk + 3 behind one leading element; NaN (-128) wherever no row lies
    host = torch.from_numpy(rows)
    flat = torch.full((1 + B * (L + 3),), -128 if kind == "int8" else float("nan"), dtype=host.dtype, device="cuda")
    view = torch.as_strided(flat, (B, L), (L + 3, 1), 1)
    view.copy_(host)
    planes = _planes(c)
    c.depuncture_device(view, planes, llr_step=step)
    _check(c, planes, wide.astype(np.float64), n, rate)
    # a copy keeps the sign of zero too
    ref = PM.reference_planes(wide.astype(np.float64), n, T.PUNCTURE_PATTERNS[rate], B)
    got = planes.cpu().numpy()[:ref.size]
    num = ~np.isnan(ref)
    assert np.array_equal(np.signbit(got[num]), np.signbit(ref[num]))
