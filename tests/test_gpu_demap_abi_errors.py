"""Argument checks of the demapper entry points (include/tdec.h: the eleven tdec_demap*
calls, tdec_noise_var_dev and the fused tdec_demap_decode_dev), through the C ABI: the
return code of every rejected call, the order in which an entry point looks at its
arguments where a caller can observe it, that a rejected call says why (tdec_last_error)
and that a rejected or empty call writes nothing (the outputs are pre-filled with NaN).
No call in the first part reaches a kernel: each is turned away by the library's own
checks.  Then one functional case per launch path, on a handle nobody has reserved.

Two answers are not what the header's "B = 0 is a no-op, null arguments are
TDEC_EINVAL" suggests, and are pinned as they are:
  - the flat and per-row calls look at their pointers before the count, so an empty
    call with a null pointer is TDEC_EINVAL (the handle calls accept null data
    pointers at B = 0, but not a null table);
  - tdec_demap_rows*_dev accept S = 0 (a no-op) where the handle calls refuse S <= 0."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulations_amd import _native as NT  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402

FLAT_DEV = ("tdec_demap_dev", "tdec_demap_logmap_dev")
FLAT_HOST = ("tdec_demap", "tdec_demap_logmap")
ROWS = ("tdec_demap_rows_dev", "tdec_demap_rows_logmap_dev")
PLANES = ("tdec_demap_planes_dev", "tdec_demap_planes_logmap_dev")
PLANES_NV = ("tdec_demap_planes_nv_dev", "tdec_demap_planes_logmap_nv_dev")
BATCH, NOISE, FUSED = "tdec_demap_batch", "tdec_noise_var_dev", "tdec_demap_decode_dev"
FLAT = FLAT_DEV + FLAT_HOST
HANDLE = PLANES + PLANES_NV + (FUSED,)             # tdec_t *h first, [B][S] symbols
TABLE = FLAT + ROWS + HANDLE + (NOISE,)            # the caller's table (BATCH has its own)
ALL = TABLE + (BATCH,)
B, S, BPS = 65, 36, 4                              # 16QAM: one full tile of codewords and one row
EINVAL = NT.TDEC_EINVAL


def _symbols():
    rng = np.random.default_rng(65)
    cons = D.constellation("16QAM")
    return (cons[rng.integers(0, 16, (B, S))] +
            0.25 * (rng.standard_normal((B, S)) + 1j * rng.standard_normal((B, S)))).astype(np.complex64)


def _nan(n, dtype=torch.float64):
    return torch.full((n,), np.nan, dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def env():
    """An N = 48 r = 1/3 handle that nobody reserves, 65 x 36 noisy 16QAM symbols on both
    sides, the complex64 table, and outputs filled with NaN (the fused call's bits: 7)
    that no test of the first part may change."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = M.DVBRCS2_Turbo(48, "1/3")
    syms = _symbols()
    e = {"c": c, "h": c.handle.h, "syms": syms, "d_syms": torch.from_numpy(syms).cuda(),
         "cons": np.ascontiguousarray(D.constellation("16QAM").astype(np.complex64)),
         "d_nv": torch.full((B,), 0.25, dtype=torch.float64, device="cuda"),
         "d_llr": _nan(B * S * BPS), "d_planes": _nan(c.planes_bytes(B) // 4, torch.float32), "d_est": _nan(B),
         "d_bits": torch.full((B, c.k_info), 7, dtype=torch.int32, device="cuda"), "d_lf": _nan(B * c.k_info),
         "llr": np.full(B * S * BPS, np.nan), "llr32": np.full(B * S * BPS, np.nan, np.float32)}
    yield e
    _untouched(e)


def _untouched(e):
    torch.cuda.synchronize()
    for k in ("d_llr", "d_planes", "d_est", "d_lf"):
        assert bool(torch.isnan(e[k]).all()), k
    assert bool((e["d_bits"] == 7).all())
    assert np.isnan(e["llr"]).all() and np.isnan(e["llr32"]).all()


def _call(e, name, n=1, *, rows_S=S, h="handle", syms="valid", cons="valid", out="valid", nv="valid", M_=16, bps=BPS,
          mod=3, sign=-1, bufs=None):
    """name(...) with valid or null pointers; n is n_sym (FLAT, BATCH) or B.  Returns the
    code, and checks that a failure left a message."""
    b = bufs or e
    host = name in FLAT_HOST or name == BATCH
    p_syms = NT.ptr(e["syms" if host else "d_syms"]) if syms == "valid" else None
    p_cons = NT.ptr(e["cons"]) if cons == "valid" else None
    p_nv = NT.ptr(e["d_nv"]) if nv == "valid" else None
    okey = {BATCH: "llr32", NOISE: "d_est", FUSED: "d_bits"}.get(name, "llr" if host else
                                                                  "d_llr" if name in FLAT + ROWS else "d_planes")
    p_out = NT.ptr(b[okey]) if out == "valid" else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lm = "logmap" in name
    div = [] if lm else [1]
    if name in FLAT:
        args = [0, p_syms, 0, n, p_cons, 0, M_, bps, 0.25, *div, sign, p_out] + ([] if host else [st])
    elif name in ROWS:
        args = [0, p_syms, 0, n, rows_S, p_cons, 0, M_, bps, p_nv, *div, sign, p_out, st]
    elif name in PLANES + PLANES_NV:
        args = [e["h"] if h == "handle" else None, n, p_syms, rows_S, p_cons, 0, M_, bps,
                p_nv if name in PLANES_NV else 0.25, *div, p_out, st]
    elif name == FUSED:
        args = [e["h"] if h == "handle" else None, n, p_syms, rows_S, p_cons, 0, M_, bps, 0.25, 1, p_out,
                NT.ptr(b["d_lf"]) if out == "valid" else None, st]
    elif name == NOISE:
        args = [0, p_syms, n, rows_S, p_cons, 0, M_, 0.02, p_out, st]
    else:
        args = [0, mod, sign, p_syms, n, 0.25, p_out]
    rc = getattr(NT.lib(), name)(*args)
    if rc != 0:
        assert NT.lib().tdec_last_error(), name
    return rc


def test_the_lists_above_are_the_thirteen_calls():
    assert len(ALL) == len(set(ALL)) == 13
    assert sorted(n for n in NT.EXPORTS if n.startswith("tdec_demap") or n == NOISE) == sorted(ALL)


@pytest.mark.parametrize("name", ALL)
def test_null_data_pointers(env, name):
    assert _call(env, name, syms=None) == EINVAL
    assert _call(env, name, out=None) == EINVAL
    assert _call(env, name, syms=None, out=None) == EINVAL


@pytest.mark.parametrize("name", TABLE)
def test_null_table(env, name):
    assert _call(env, name, cons=None) == EINVAL
    assert _call(env, name, 0, cons=None) == EINVAL          # before the empty batch, on every call
    assert _call(env, name, 0, cons=None, syms=None, out=None) == EINVAL


@pytest.mark.parametrize("name", HANDLE)
def test_null_handle(env, name):
    assert _call(env, name, h=None) == EINVAL
    assert _call(env, name, 0, h=None) == EINVAL
    assert _call(env, name, 0, h=None, syms=None, out=None) == EINVAL


@pytest.mark.parametrize("name", ROWS)
def test_null_noise_var_on_the_flat_row_forms_comes_first(env, name):
    assert _call(env, name, nv=None) == EINVAL
    assert _call(env, name, 0, nv=None) == EINVAL
    assert _call(env, name, 1, rows_S=0, nv=None) == EINVAL


@pytest.mark.parametrize("name", PLANES_NV)
def test_null_noise_var_on_the_plane_forms_comes_after_the_empty_batch(env, name):
    assert _call(env, name, nv=None) == EINVAL
    assert _call(env, name, B, nv=None) == EINVAL
    assert _call(env, name, 0, nv=None) == 0
    assert _call(env, name, 0, nv=None, syms=None, out=None) == 0


@pytest.mark.parametrize("name", ALL)
def test_negative_count(env, name):
    assert _call(env, name, -1) == EINVAL
    assert _call(env, name, -1, syms=None, out=None) == EINVAL


@pytest.mark.parametrize("name", ALL)
def test_empty_call_writes_nothing(env, name):
    assert _call(env, name, 0) == 0
    _untouched(env)


@pytest.mark.parametrize("name", FLAT + ROWS)
def test_flat_forms_look_at_their_pointers_before_the_count(env, name):
    assert _call(env, name, 0, syms=None) == EINVAL
    assert _call(env, name, 0, out=None) == EINVAL
    assert _call(env, name, 0, syms=None, out=None) == EINVAL


@pytest.mark.parametrize("name", HANDLE + (NOISE, BATCH))
def test_empty_batch_is_a_no_op_with_null_data_pointers(env, name):
    assert _call(env, name, 0, syms=None, out=None) == 0
    assert _call(env, name, 0, syms=None, out=None, rows_S=0) == 0
    assert _call(env, name, 0, syms=None, out=None, rows_S=-1) == 0


@pytest.mark.parametrize("name", ROWS)
def test_row_forms_accept_no_symbols_per_row(env, name):
    assert _call(env, name, B, rows_S=0) == 0
    assert _call(env, name, 0, rows_S=0) == 0
    assert _call(env, name, B, rows_S=-1) == EINVAL
    assert _call(env, name, 0, rows_S=-1) == EINVAL           # before the empty batch
    _untouched(env)


@pytest.mark.parametrize("name", HANDLE + (NOISE,))
def test_handle_forms_and_the_estimator_refuse_no_symbols_per_row(env, name):
    assert _call(env, name, 1, rows_S=0) == EINVAL
    assert _call(env, name, B, rows_S=-1) == EINVAL
    assert _call(env, name, 0, rows_S=0) == 0                 # after the empty batch
    assert _call(env, name, 0, rows_S=-1) == 0


@pytest.mark.parametrize("M_,bps", [(17, 4), (16, 0), (16, 9), (0, 4), (257, 8), (16, -1)])
@pytest.mark.parametrize("name", FLAT + ROWS + HANDLE)
def test_bad_constellation_size(env, name, M_, bps):
    assert _call(env, name, M_=M_, bps=bps) == EINVAL
    assert b"constellation" in NT.lib().tdec_last_error()
    assert _call(env, name, 0, M_=M_, bps=bps) == EINVAL      # before the empty batch
    if name in HANDLE:
        assert _call(env, name, 0, M_=M_, bps=bps, syms=None, out=None) == EINVAL


def test_the_estimator_derives_bps_from_the_table_size(env):
    """No bps argument: M = 0 and M > 256 are refused (before the empty batch), any M in
    1..256 has a bps that holds it (17 points are a 5-bit table)."""
    for M_ in (0, -1, 257):
        assert _call(env, NOISE, M_=M_) == EINVAL
        assert b"constellation" in NT.lib().tdec_last_error()
        assert _call(env, NOISE, 0, M_=M_, syms=None, out=None) == EINVAL
    assert _call(env, NOISE, 0, M_=17) == 0
    assert _call(env, NOISE, 1, M_=17, out=None) == EINVAL


def test_fixed_signature_demapper(env):
    """tdec_demap_batch: the modulation id, then count and sign, then the empty call, then
    the pointers."""
    assert _call(env, BATCH, mod=6) == EINVAL
    assert b"modulation" in NT.lib().tdec_last_error()
    assert _call(env, BATCH, 0, mod=-1, syms=None, out=None) == EINVAL
    assert _call(env, BATCH, sign=0) == EINVAL
    assert _call(env, BATCH, 0, sign=2, syms=None, out=None) == EINVAL
    assert _call(env, BATCH, 0, syms=None, out=None) == 0


def test_fused_call_after_its_pointers(env):
    """tdec_demap_decode_dev: no kernel for this (algorithm, table) pair is
    TDEC_EUNSUPPORTED, a handle tdec_reserve_fused has not sized TDEC_ECAPACITY; both
    come after the pointer checks and write nothing."""
    assert _call(env, FUSED, M_=8, bps=3) == NT.TDEC_EUNSUPPORTED
    assert _call(env, FUSED, M_=8, bps=3, out=None) == EINVAL
    assert _call(env, FUSED, 0, M_=8, bps=3, syms=None, out=None) == 0
    assert _call(env, FUSED, B) == NT.TDEC_ECAPACITY
    assert _call(env, FUSED, B, syms=None) == EINVAL
    assert _call(env, FUSED, B, rows_S=0) == EINVAL
    _untouched(env)


# ---- one functional case per launch path --------------------------------------------------
def _flat(e, name, n, out, **kw):
    assert _call(e, name, n, bufs={"d_llr": out, "llr": out}, **kw) == 0
    return out


@pytest.fixture(scope="module")
def flat_llr(env):
    """tdec_demap_dev / tdec_demap_logmap_dev (sign -1, noise_var 0.25, f32 division) over
    the 65 x 36 symbols: the reference of the other flat forms and of the planes."""
    return {lm: _flat(env, FLAT_DEV[lm], B * S, torch.zeros(B * S * BPS, dtype=torch.float64, device="cuda"))
            for lm in (0, 1)}


@pytest.mark.parametrize("lm", [0, 1])
def test_flat_forms_agree_bit_for_bit(env, flat_llr, lm):
    ref = flat_llr[lm]
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1.0
    rows = _flat(env, ROWS[lm], B, _nan(B * S * BPS))                  # a constant vector
    assert torch.equal(rows.view(torch.int64), ref.view(torch.int64))
    host = np.full(B * S * BPS, np.nan)
    _flat(env, FLAT_HOST[lm], B * S, host)
    assert np.array_equal(host.view(np.int64), ref.cpu().numpy().view(np.int64))
    one = _flat(env, ROWS[lm], 1, _nan(S * BPS))                       # then a single row
    assert torch.equal(one.view(torch.int64), ref[:S * BPS].view(torch.int64))
    one = _flat(env, FLAT_DEV[lm], S, _nan(S * BPS))
    assert torch.equal(one.view(torch.int64), ref[:S * BPS].view(torch.int64))


def test_fixed_signature_demapper_is_the_flat_demapper_rounded(env, flat_llr):
    out = np.full(B * S * BPS, np.nan, np.float32)
    assert _call(env, BATCH, B * S, bufs={"llr32": out}) == 0
    assert np.array_equal(out.view(np.int32), flat_llr[0].cpu().numpy().astype(np.float32).view(np.int32))


def _planes(e, name, n):
    out = torch.full((e["c"].planes_bytes(n) // 4,), 7.0, dtype=torch.float32, device="cuda")
    assert _call(e, name, n, bufs={"d_planes": out}) == 0
    return out


@pytest.fixture(scope="module")
def plane_results(env):
    """The four plane forms at B = 65 and then B = 1 on the handle as created: the first
    max-log call grows the decline list (16QAM is a split table) to two tiles itself.
    Only afterwards is the handle reserved, for the de-puncture kernel of the reference."""
    c = env["c"]
    got = {(name, n): _planes(env, name, n) for n in (B, 1) for name in PLANES + PLANES_NV}
    torch.cuda.synchronize()
    c.reserve(B)
    return got


@pytest.mark.parametrize("n", [B, 1])
@pytest.mark.parametrize("lm", [0, 1])
def test_planes_equal_flat_demap_then_depuncture(env, flat_llr, plane_results, lm, n):
    c = env["c"]
    L = c.handle.llr_len
    assert S * BPS < L                                                # the symbols end early: zero LLRs follow
    rows = torch.zeros((n, L), dtype=torch.float32, device="cuda")
    rows[:, :S * BPS] = flat_llr[lm].to(torch.float32).reshape(B, S * BPS)[:n]
    ref = torch.full_like(plane_results[PLANES[lm], n], 7.0)
    c.depuncture_device(rows, ref)
    assert torch.equal(plane_results[PLANES[lm], n].view(torch.int32), ref.view(torch.int32))
    # noise_var[row] with a constant vector: the scalar call bit for bit
    assert torch.equal(plane_results[PLANES_NV[lm], n].view(torch.int32), ref.view(torch.int32))


def test_estimator_runs_after_the_rejected_calls(env):
    est = _nan(B)
    assert _call(env, NOISE, B, bufs={"d_est": est}) == 0
    one = _nan(1)
    assert _call(env, NOISE, 1, bufs={"d_est": one}) == 0
    assert bool(torch.isfinite(est).all()) and bool((est >= 0.02).all()) and float(est.max()) < 1.0
    assert torch.equal(one.view(torch.int64), est[:1].view(torch.int64))
