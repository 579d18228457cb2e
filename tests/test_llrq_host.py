"""Quantised LLRs without a GPU: the restatement's own properties
(tests/llrq_ref.py), the default step, the BER tool's sweep configuration, and the C ABI's
bookkeeping (include/llrq.h against the binding list and the built library's exports)."""
import argparse
import os
import re

import numpy as np
import pytest

import llrq_ref as Q
from modulations_amd import _native, ber

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -------------------------------------------------------------------------

def test_ties_round_to_even_and_the_ends_saturate():
    one = np.float32(1)   # step 1: the products are the inputs
    x = np.float32([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -126.5, 127.5, -127.5, np.inf, -np.inf, 127.0, -127.0,
                    128.0, -128.0, 1e30, -1e30])
    want = np.int8([0, 0, 2, -2, 2, -2, 126, -126, 127, -127, 127, -127, 127, -127, 127, -127, 127, -127])
    assert np.array_equal(Q.quantize(x, one), want)
    assert Q.saturated(x, one) == 8      # +-127.5, +-inf, +-128, +-1e30; 127 itself is not


def test_ties_in_steps_of_a_power_of_two_step():
    step = np.float32(0.25)   # exact products: the ties are ties
    x = np.float32([0.5, 1.5, 2.5, -0.5, -1.5, -2.5]) * step
    assert np.array_equal(Q.quantize(x, step), np.int8([0, 2, 2, 0, -2, -2]))


def test_nan_is_an_erasure_and_minus_zero_is_zero():
    q = Q.quantize(np.float32([np.nan, -np.nan, -0.0, 0.0, 1e-45, -1e-45]))
    assert np.array_equal(q, np.zeros(6, np.int8))
    assert Q.saturated(np.float32([np.nan, -0.0])) == 0


def test_float64_is_rounded_to_float32_first():
    # 2.5 + 2^-30 is above the tie as a float64 (-> 3) and on it as a float32 (-> 2, to even)
    x = np.float64(2.5) + np.float64(2.0) ** -30
    assert np.float32(x) == np.float32(2.5) and x > 2.5
    assert Q.quantize(np.array([x]), np.float32(1))[0] == 2
    assert np.rint(x) == 3.0
    # and the product is a float32 one: the step is not widened either
    assert Q.quantize(np.array([x, -x]), np.float32(1)).dtype == np.int8


def test_round_trip_is_within_half_a_step():
    rng = np.random.default_rng(17)
    for step in (Q.DEFAULT_STEP, np.float32(30 / 31), np.float32(0.125), np.float32(0.3)):
        lim = np.float32(127) * step
        x = np.concatenate([rng.uniform(-lim, lim, 20000).astype(np.float32), np.float32([lim, -lim, 0.0])])
        x = x[np.abs(x) <= lim]
        back = Q.dequantize_i8(Q.quantize(x, step), step)
        assert np.max(np.abs(back.astype(np.float64) - x.astype(np.float64))) <= float(step) / 2


def test_dequantize_i8_takes_minus_128():
    step = np.float32(0.3)
    got = Q.dequantize_i8(np.int8([-128, 127, 0, -1]), step)
    assert got.dtype == np.float32
    assert np.array_equal(got, np.float32([-128, 127, 0, -1]) * step)
    assert got[0] == np.float32(-128) * step and not np.signbit(got[2])


def test_dequantize_f16_is_exact():
    h = np.array([np.inf, -np.inf, np.nan, 65504.0, 6e-8, -6e-8, -0.0, 1.0009765625], np.float16)
    got = Q.dequantize_f16(h)
    assert got.dtype == np.float32
    assert np.array_equal(got.astype(np.float16).view(np.uint16), h.view(np.uint16))   # nothing lost
    assert got[4] != 0 and np.isnan(got[2]) and np.signbit(got[6])                     # subnormal kept


def test_default_step():
    assert _native.LLRQ_DEFAULT_STEP.dtype == np.float32
    assert _native.LLRQ_DEFAULT_STEP == np.float32(30 / 127) == Q.DEFAULT_STEP
    from modulations_amd import demap
    from modulations_amd.dvb_rcs2_turbo import llr_step_arg
    assert demap.LLR_DEFAULT_STEP == Q.DEFAULT_STEP
    assert llr_step_arg("int8", None) == Q.DEFAULT_STEP and llr_step_arg("f16", None) == np.float32(1)
    assert llr_step_arg("int8", 0.3) == np.float32(0.3)
    with pytest.raises(TypeError):
        llr_step_arg("f16", 0.5)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            llr_step_arg("int8", bad)
    # +-30, where compute_llr clips, is the last code
    assert np.array_equal(Q.quantize(np.float32([30.0, -30.0])), np.int8([127, -127]))


# ---- the BER tool's sweep configuration --------------------------------------------------------

def _cfg(*argv):
    return ber.sweep_config(ber.arg_parser().parse_args(list(argv)))


def test_sweep_config_records_the_link_only_when_it_is_not_f32():
    plain = _cfg()
    assert _cfg("--llr", "f32") == plain
    assert "llr" not in plain and "llr_step" not in plain
    # a namespace of the parent's parser (no llr attributes at all) gives the same configuration
    ns = vars(ber.arg_parser().parse_args([]))
    assert ber.sweep_config(argparse.Namespace(**{k: v for k, v in ns.items() if k not in ("llr", "llr_step")})) == plain
    q = _cfg("--llr", "int8")
    assert {k: v for k, v in q.items() if k not in ("llr", "llr_step")} == plain
    assert q["llr"] == "int8" and q["llr_step"] == float(np.float32(30 / 127))
    assert set(q) - set(plain) == {"llr", "llr_step"}
    coarse = _cfg("--llr", "int8", "--llr-step", str(30 / 31))
    assert coarse["llr_step"] == float(np.float32(30 / 31)) and coarse != q
    h = _cfg("--llr", "f16")
    assert h["llr"] == "f16" and h["llr_step"] == 1.0


def test_resume_with_another_link_is_refused(tmp_path):
    out = str(tmp_path / "ber.json")
    ber.save_results(out, _cfg(), [{"ebn0_db": 0.0}])
    assert 0.0 in ber.load_resume(out, _cfg("--llr", "f32"))
    for other in (("--llr", "int8"), ("--llr", "f16")):
        with pytest.raises(ValueError):
            ber.load_resume(out, _cfg(*other))


# ---- the C ABI's bookkeeping ---------------------------------------------------------------------

def _llrq_header_symbols():
    src = open(os.path.join(ROOT, "include", "llrq.h")).read()
    return sorted(set(re.findall(r"^\s*(?:[\w\s\*]+?)\b(llrq_\w+)\s*\(", src, re.M)))


def test_llrq_header_matches_binding_list():
    assert _llrq_header_symbols() == sorted(_native.LLRQ_EXPORTS)
    assert len(_native.LLRQ_EXPORTS) == 5
    assert not set(_native.LLRQ_EXPORTS) & (set(_native.EXPORTS) | set(_native.HARQ_EXPORTS) | set(_native.CRC_EXPORTS))
    src = open(os.path.join(ROOT, "include", "llrq.h")).read()
    assert not re.findall(r"^\s*(?:[\w\s\*]+?)\b(tdec_\w+)\s*\(", src, re.M)    # llrq.h declares no tdec_ call
    assert _native.LLRQ_KINDS == {"int8": 0, "f16": 1}
    assert re.search(r"LLRQ_INT8 = 0, LLRQ_F16 = 1", src)


def test_library_exports_the_llrq_symbols():
    import ctypes as C
    import subprocess
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in _native.LLRQ_EXPORTS:
        assert re.search(rf"\bT {name}$", out, re.M), name
        assert getattr(lib, name).restype is C.c_int
    assert [a.__name__ for a in lib.llrq_quantize_dev.argtypes] == \
        ["c_int", "c_void_p", "c_int", "c_long", "c_float", "c_void_p", "c_void_p", "c_void_p"]
    assert [a.__name__ for a in lib.llrq_depuncture_dev.argtypes] == \
        ["c_void_p", "c_int", "c_void_p", "c_int", "c_float", "c_long", "c_void_p", "c_void_p"]
    assert [a.__name__ for a in lib.llrq_depuncture_acc_dev.argtypes] == \
        ["c_void_p", "c_int", "c_void_p", "c_int", "c_float", "c_long", "c_int", "c_void_p", "c_void_p", "c_void_p"]
    assert [a.__name__ for a in lib.llrq_decode_dev.argtypes] == \
        ["c_void_p", "c_int", "c_int", "c_void_p", "c_int", "c_float", "c_long", "c_void_p", "c_void_p", "c_void_p",
         "c_void_p"]
    assert [a.__name__ for a in lib.llrq_decode_batch.argtypes] == \
        ["c_void_p", "c_int", "c_void_p", "c_int", "c_float", "c_long", "c_void_p", "c_void_p"]
