"""ctypes bindings of the gfx950 HIP libraries (modulations_amd/lib/libtdec.so:
turbo decoder + soft demapper; modulations_amd/lib/libmodem.so: modem front-end).

The product path has no CPU fallback: if the library is missing or no HIP
device is visible, calls raise instead of computing anything on the host.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libtdec.so")
# A/B experiments only: TDEC_LIB_VARIANT=w4 loads lib/libtdec_w4.so (built by build.py --variant)
if os.environ.get("TDEC_LIB_VARIANT"):
    LIB_PATH = os.path.join(HERE, "lib", f"libtdec_{os.environ['TDEC_LIB_VARIANT']}.so")

TDEC_OK, TDEC_EINVAL, TDEC_ESHORT, TDEC_ENOMEM, TDEC_EHIP, TDEC_EUNSUPPORTED, TDEC_EITER, TDEC_ECAPACITY = \
    0, -1, -2, -3, -4, -5, -6, -7

# every symbol include/tdec.h declares (tests check the library exports them all)
EXPORTS = (
    "tdec_create", "tdec_destroy", "tdec_last_error", "tdec_llr_len", "tdec_siso_batch", "tdec_decode_batch",
    "tdec_reserve", "tdec_planes_bytes", "tdec_depuncture_dev", "tdec_decode_planes_dev", "tdec_decode_batch_dev",
    "tdec_tail_gate",
    "tdec_demap_dev", "tdec_demap", "tdec_demap_planes_dev", "tdec_encode_dev", "tdec_encoded_len",
    "tdec_demap_batch", "tdec_constellation", "tdec_workload_dev", "tdec_info_bits_dev", "tdec_count_errors_dev",
    "tdec_reserve_fused", "tdec_fused_available", "tdec_demap_decode_dev", "tdec_selftest", "tdec_selftest_trans",
    "tdec_host_alloc", "tdec_host_free", "tdec_encode_host", "tdec_siso_batch_f64", "tdec_siso_staging",
    "tdec_siso_staged", "tdec_siso_stats",
    "tdec_decode_batch_es", "tdec_decode_planes_es_dev", "tdec_decode_batch_es_dev", "tdec_es_capacity",
    "tdec_early_stop_available",
    "tdec_decode_batch_es_tile", "tdec_decode_planes_es_tile_dev", "tdec_decode_batch_es_tile_dev",
    "tdec_reserve_es_refill", "tdec_decode_batch_es_refill", "tdec_decode_planes_es_refill_dev",
    "tdec_decode_batch_es_refill_dev", "tdec_es_refill_stats",
    "tdec_demap_logmap_dev", "tdec_demap_logmap", "tdec_demap_planes_logmap_dev",
    "tdec_noise_var_dev", "tdec_demap_rows_dev", "tdec_demap_rows_logmap_dev", "tdec_demap_planes_nv_dev",
    "tdec_demap_planes_logmap_nv_dev",
    "tdec_symnv_demap_dev", "tdec_symnv_demap_logmap_dev", "tdec_symnv_demap_planes_dev",
    "tdec_symnv_demap_planes_logmap_dev", "tdec_equalize_dev", "tdec_workload_fading_dev",
    "tdec_csi_pilots_dev", "tdec_csi_strip_dev", "tdec_workload_frame_dev",
    "tdec_combine_dev", "tdec_workload_branches_dev", "tdec_workload_frame_branches_dev",
)

_lib = None
_lock = threading.Lock()

_vp = C.c_void_p


def _declare(L):
    """argtypes and restype of every export the loaded library has: the A/B tools also load older builds
    through this, and an export such a build lacks is skipped."""
    i, l, d, p, q, Q, z, ptr = C.c_int, C.c_long, C.c_double, _vp, C.c_int64, C.c_uint64, C.c_size_t, C.POINTER
    siso = [p, i, p, p, p, p, p, p, d, p, p]
    batch, batch_es, planes_es = [p, i, p, l, p, p], [p, i, p, l, p, p, p], [p, i, p, p, p, p, p]
    flat = [i, p, i, l, p, i, i, i, d]                    # the flat demappers up to their scalar noise_var
    rows = [i, p, i, i, i, p, i, i, i, p]                 # their per-row and per-symbol forms up to the tensor
    planes = [p, i, p, i, p, i, i, i]                     # the plane demappers up to M, bps
    symbols = [p, i, q, Q, p, i, i, d]                    # the symbol generators up to sigma
    frame = [i, i, i, i, p, d, q, Q, d, p, p, p]          # the framing generators from S on
    argtypes = {
        "tdec_create": [i, i, i, p, i, i, p, p, p, ptr(p)], "tdec_destroy": [p], "tdec_last_error": [],
        "tdec_llr_len": [p], "tdec_encoded_len": [p], "tdec_reserve": [p, i], "tdec_planes_bytes": [p, i],
        "tdec_siso_batch": siso, "tdec_siso_batch_f64": siso, "tdec_siso_staging": [p, i, ptr(p), ptr(z)],
        "tdec_siso_staged": [p, i, i, d], "tdec_siso_stats": [p, ptr(l)],
        "tdec_depuncture_dev": batch, "tdec_tail_gate": [p, p],
        "tdec_decode_batch": batch, "tdec_decode_planes_dev": [p, i, p, p, p, p], "tdec_decode_batch_dev": batch + [p],
        "tdec_decode_batch_es": batch_es, "tdec_decode_planes_es_dev": planes_es,
        "tdec_decode_batch_es_dev": batch_es + [p], "tdec_es_capacity": [p], "tdec_early_stop_available": [i],
        "tdec_decode_batch_es_tile": batch_es, "tdec_decode_planes_es_tile_dev": planes_es,
        "tdec_decode_batch_es_tile_dev": batch_es + [p],
        "tdec_reserve_es_refill": [p, i], "tdec_decode_batch_es_refill": batch_es,
        "tdec_decode_planes_es_refill_dev": planes_es, "tdec_decode_batch_es_refill_dev": batch_es + [p],
        "tdec_es_refill_stats": [p, ptr(l), ptr(l)],
        "tdec_demap_dev": flat + [i, i, p, p], "tdec_demap": flat + [i, i, p],
        "tdec_demap_logmap_dev": flat + [i, p, p], "tdec_demap_logmap": flat + [i, p],
        "tdec_demap_rows_dev": rows + [i, i, p, p], "tdec_demap_rows_logmap_dev": rows + [i, p, p],
        "tdec_symnv_demap_dev": rows + [i, i, p, p], "tdec_symnv_demap_logmap_dev": rows + [i, p, p],
        "tdec_demap_planes_dev": planes + [d, i, p, p], "tdec_demap_planes_logmap_dev": planes + [d, p, p],
        "tdec_demap_planes_nv_dev": planes + [p, i, p, p], "tdec_demap_planes_logmap_nv_dev": planes + [p, p, p],
        "tdec_symnv_demap_planes_dev": planes + [p, i, p, p], "tdec_symnv_demap_planes_logmap_dev": planes + [p, p, p],
        "tdec_reserve_fused": [p, i], "tdec_fused_available": [p, i, i],
        "tdec_demap_decode_dev": planes + [d, i, p, p, p],
        "tdec_demap_batch": [i, i, i, p, l, C.c_float, p], "tdec_constellation": [i, p, ptr(i)],
        "tdec_noise_var_dev": [i, p, i, i, p, i, i, d, p, p],
        "tdec_equalize_dev": [i, p, p, i, i, i, d, p, p, p, p],
        "tdec_combine_dev": [i, p, p, i, i, i, i, d, p, p, p, p, p],
        "tdec_csi_pilots_dev": [i, p, i, i, i, i, p, i, d, p, d, p, p, p, p, p],
        "tdec_csi_strip_dev": [i, p, i, i, i, i, p, i, d, p, p, p, p],
        "tdec_encode_dev": [p, i, p, p, p], "tdec_encode_host": [i, i, p, p, l, p, l, p, l],
        "tdec_info_bits_dev": [p, i, q, Q, p, p], "tdec_count_errors_dev": [p, i, q, Q, p, p, p],
        "tdec_workload_dev": symbols + [p, p, p], "tdec_workload_fading_dev": symbols + [d, i, p, p, p, p],
        "tdec_workload_branches_dev": [p, i, i, q, Q, p, i, i, d, d, i, p, p, p, p],
        "tdec_workload_frame_dev": [i, p, p, i] + frame, "tdec_workload_frame_branches_dev": [i, p, p, i, i] + frame,
        "tdec_selftest": [i, i, C.c_longlong, C.c_ulonglong, ptr(C.c_longlong)],
        "tdec_selftest_trans": [i, i, C.c_uint32, C.c_longlong, p],
        "tdec_host_alloc": [z, ptr(p)], "tdec_host_free": [p],
    }
    # int (a status, or a small count) is what every export returns but these
    restype = {"tdec_destroy": None, "tdec_host_free": None, "tdec_last_error": C.c_char_p, "tdec_llr_len": l,
               "tdec_encoded_len": l, "tdec_encode_host": l, "tdec_planes_bytes": z}
    for name in EXPORTS:
        if hasattr(L, name):
            f = getattr(L, name)
            f.argtypes, f.restype = argtypes[name], restype.get(name, i)


# every symbol include/harq.h declares (hybrid ARQ): built into libtdec.so,
# kept apart from EXPORTS as MODEM_EXPORTS is
HARQ_EXPORTS = ("harq_depuncture_acc_dev", "harq_workload_tx_dev")


def _declare_harq(L):
    """argtypes and restype of include/harq.h's exports; a library that lacks them (an older
    build loaded by the A/B tools) is left as it is, and a call then fails by name."""
    i, l, d, p, q, Q = C.c_int, C.c_long, C.c_double, _vp, C.c_int64, C.c_uint64
    argtypes = {
        "harq_depuncture_acc_dev": [p, i, p, i, l, i, p, p, p],
        "harq_workload_tx_dev": [p, i, i, q, Q, p, i, i, d, i, d, i, p, p, p, p],
    }
    for name in HARQ_EXPORTS:
        if hasattr(L, name):
            f = getattr(L, name)
            f.argtypes, f.restype = argtypes[name], i


# every symbol include/crc.h declares (frame check): built into libtdec.so,
# kept apart as HARQ_EXPORTS is
CRC_EXPORTS = ("crc_attach_dev", "crc_check_dev", "crc_check_u8_dev", "crc_workload_tx_dev")
CRC_KINDS = {"crc16": 16, "crc32": 32}          # the header's CRC_KIND16 / CRC_KIND32: the width r


def _declare_crc(L):
    """argtypes and restype of include/crc.h's exports; a library that lacks them (an older
    build loaded by the A/B tools) is left as it is, and a call then fails by name."""
    i, l, d, p, q, Q = C.c_int, C.c_long, C.c_double, _vp, C.c_int64, C.c_uint64
    argtypes = {
        "crc_attach_dev": [i, i, l, i, p, p],
        "crc_check_dev": [i, i, l, i, p, p, p, p],
        "crc_check_u8_dev": [i, i, l, i, p, p, p, p],
        "crc_workload_tx_dev": [p, i, i, q, Q, p, i, i, d, i, d, i, p, p, p, p],
    }
    for name in CRC_EXPORTS:
        if hasattr(L, name):
            f = getattr(L, name)
            f.argtypes, f.restype = argtypes[name], i


# every symbol include/llrq.h declares (quantised channel LLRs): built into
# libtdec.so, kept apart as HARQ_EXPORTS is
LLRQ_EXPORTS = ("llrq_quantize_dev", "llrq_depuncture_dev", "llrq_depuncture_acc_dev", "llrq_decode_dev",
                "llrq_decode_batch")
LLRQ_KINDS = {"int8": 0, "f16": 1}              # the header's LLRQ_INT8 / LLRQ_F16
LLRQ_MODES = {None: 0, "frame": 1, "tile": 2, "refill": 3}   # LLRQ_DEC_*: fixed iterations, or early stop by es_decoder
LLRQ_DEFAULT_STEP = np.float32(30 / 127)        # compute_llr clips to +-30


def _declare_llrq(L):
    """argtypes and restype of include/llrq.h's exports; a library that lacks them (an older
    build loaded by the A/B tools) is left as it is, and a call then fails by name."""
    i, l, f, p = C.c_int, C.c_long, C.c_float, _vp
    argtypes = {
        "llrq_quantize_dev": [i, p, i, l, f, p, p, p],
        "llrq_depuncture_dev": [p, i, p, i, f, l, p, p],
        "llrq_depuncture_acc_dev": [p, i, p, i, f, l, i, p, p, p],
        "llrq_decode_dev": [p, i, i, p, i, f, l, p, p, p, p],
        "llrq_decode_batch": [p, i, p, i, f, l, p, p],
    }
    for name in LLRQ_EXPORTS:
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes[name], i


# every symbol include/stbc.h declares (transmit diversity): built into
# libtdec.so, kept apart as HARQ_EXPORTS is
STBC_EXPORTS = ("stbc_combine_dev", "stbc_workload_dev")


def _declare_stbc(L):
    """argtypes and restype of include/stbc.h's exports; a library that lacks them (an older
    build loaded by the A/B tools) is left as it is, and a call then fails by name."""
    i, d, p, q, Q = C.c_int, C.c_double, _vp, C.c_int64, C.c_uint64
    argtypes = {
        "stbc_combine_dev": [i, p, p, i, i, i, i, d, p, p, p, p, p],
        "stbc_workload_dev": [p, i, i, q, Q, p, i, i, d, d, i, p, p, p, p],
    }
    for name in STBC_EXPORTS:
        if hasattr(L, name):
            f = getattr(L, name)
            f.argtypes, f.restype = argtypes[name], i


# every symbol include/sm.h declares (spatial multiplexing): built into
# libtdec.so, kept apart as STBC_EXPORTS is
SM_EXPORTS = ("sm_detect_dev", "sm_workload_dev")


def _declare_sm(L):
    """argtypes and restype of include/sm.h's exports; a library that lacks them (an older
    build loaded by the A/B tools) is left as it is, and a call then fails by name."""
    i, d, p, q, Q, l = C.c_int, C.c_double, _vp, C.c_int64, C.c_uint64, C.c_long
    argtypes = {
        "sm_detect_dev": [i, p, p, i, i, i, i, p, i, i, d, p, p, i, p, l, p],
        "sm_workload_dev": [p, i, i, q, Q, p, i, i, d, d, i, p, p, p, p],
    }
    for name in SM_EXPORTS:
        if hasattr(L, name):
            f = getattr(L, name)
            f.argtypes, f.restype = argtypes[name], i


def lib():
    """Load libtdec.so (building it first if this is a build tree without it)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    from . import build
                    build.build()
                L = C.CDLL(LIB_PATH)
                _declare(L)
                _declare_harq(L)
                _declare_crc(L)
                _declare_llrq(L)
                _declare_stbc(L)
                _declare_sm(L)
                _lib = L
    return _lib


class TdecError(RuntimeError):
    pass


def check(rc):
    if rc == TDEC_OK:
        return
    msg = lib().tdec_last_error().decode(errors="replace")
    if rc == TDEC_EINVAL or rc == TDEC_EUNSUPPORTED:
        raise ValueError(msg)
    if rc == TDEC_ESHORT:
        raise IndexError(msg)
    if rc == TDEC_ENOMEM:
        raise MemoryError(msg)
    if rc == TDEC_EITER:
        raise UnboundLocalError(msg)
    raise TdecError(f"tdec error {rc}: {msg}")


def ptr(a):
    """Device or host address of a numpy array / torch tensor (None -> NULL)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


def stream_ptr(stream):
    if stream is None:
        return None
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


# ---------------------------------------------------------------- libmodem.so ----------
MODEM_LIB_PATH = os.path.join(HERE, "lib", "libmodem.so")
MDM_ENAN = -8
# every symbol include/modem.h declares
MODEM_EXPORTS = (
    "mdm_map_dev", "mdm_map", "mdm_demod_dev", "mdm_demod", "mdm_fir_dev", "mdm_fir",
    "mdm_iq_quantize_dev", "mdm_iq_quantize", "mdm_iq_dequantize_dev", "mdm_iq_dequantize", "mdm_last_error",
    "mdm_mix_dev", "mdm_mix", "mdm_burst_find_dev", "mdm_burst_find", "mdm_xcorr_peak_dev", "mdm_xcorr_peak",
    "mdm_carrier_dev", "mdm_carrier",
)
_mlib = None


def _declare_modem(L):
    """argtypes and restype of every export of include/modem.h.  A _dev form takes its host form's
    arguments and then a stream, after the NaN counter (demod) or the scratch (iq_quantize) where it has one."""
    i, l, d, p = C.c_int, C.c_long, C.c_double, _vp
    host = {
        "mdm_map": [i, p, l, i, p, i, p], "mdm_demod": [i, i, p, i, l, i, p, d, p, i, p],
        "mdm_fir": [i, p, i, l, p, i, i, i, l, l, p], "mdm_iq_quantize": [i, p, i, l, p],
        "mdm_iq_dequantize": [i, p, l, p], "mdm_mix": [i, p, i, l, l, p, d, d, p],
        "mdm_carrier": [i, p, i, l, p, p, p, p, p, p],
    }
    burst, xcorr = [i, p, i, l, p, i, l], [i, p, l, p, i, p]   # the two with other outputs: up to preamble_len, corr
    argtypes = {
        "mdm_last_error": [], **host, **{n + "_dev": a + [p] for n, a in host.items()},
        "mdm_demod_dev": host["mdm_demod"] + [p, p], "mdm_iq_quantize_dev": host["mdm_iq_quantize"] + [p, p],
        "mdm_burst_find": burst + [p, p, p], "mdm_burst_find_dev": burst + [p, p, p, p],   # dev: smooth, result, ...
        "mdm_xcorr_peak": xcorr + [p, p], "mdm_xcorr_peak_dev": xcorr + [p, p, p],         # ... scratch, stream
    }
    for name in MODEM_EXPORTS:   # int (a status) is what every export returns but the message
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes[name], C.c_char_p if name == "mdm_last_error" else i


def modem_lib():
    """Load libmodem.so (building it first if this is a build tree without it)."""
    global _mlib
    if _mlib is None:
        with _lock:
            if _mlib is None:
                if not os.path.exists(MODEM_LIB_PATH):
                    from . import build
                    build.build_modem()
                L = C.CDLL(MODEM_LIB_PATH)
                _declare_modem(L)
                _mlib = L
    return _mlib


def modem_check(rc):
    if rc == TDEC_OK:
        return
    msg = modem_lib().mdm_last_error().decode(errors="replace")
    if rc in (TDEC_EINVAL, MDM_ENAN):
        raise ValueError(msg)
    if rc == TDEC_ENOMEM:
        raise MemoryError(msg)
    raise TdecError(f"modem error {rc}: {msg}")
