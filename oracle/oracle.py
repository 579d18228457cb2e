"""ctypes front-end of the C oracle (tdec_oracle.c).

TEST INFRASTRUCTURE ONLY -- the parity checker and the "port" CPU baseline.
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import
this module; the product package never does.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "liboracle_tdec.so")
_lib = None

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


def build():
    subprocess.run(["make", "-s", "-C", _HERE], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build()
        L = C.CDLL(_SO)
        L.orc_trellis.argtypes = [_i32p, _i32p]
        L.orc_interleaver.argtypes = [C.c_int, _i32p, _i32p, _i32p]
        L.orc_siso.argtypes = [C.c_int, _f32p, _f32p, _f32p, _f32p, _f64p, _f64p, _i32p,
                               C.c_double, C.c_int, _f64p, _f64p]
        L.orc_siso64.argtypes = [C.c_int, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p,
                                 C.c_double, C.c_int, _f64p, _f64p]
        L.orc_decode.argtypes = [C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _i32p, _i32p, _i32p,
                                 _f32p, C.c_long, _i32p, C.c_void_p]
        L.orc_decode.restype = C.c_int
        L.orc_decode_batch.argtypes = [C.c_int, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _i32p, _i32p,
                                       _i32p, _f32p, C.c_long, C.c_long, _i32p, C.c_void_p, C.c_int]
        L.orc_decode_batch.restype = C.c_int
        L.orc_siso_depths.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _f64p, _f64p,
                                      _i32p, C.c_double, C.c_int, _i32p]
        L.orc_siso_depths.restype = C.c_int
        L.orc_decode_depths.argtypes = [C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _i32p, _i32p, _i32p,
                                        _f32p, C.c_long, _i32p]
        L.orc_decode_depths.restype = C.c_int
        L.orc_depuncture.argtypes = [C.c_int, C.c_int, _u8p, _f32p, C.c_long, _f32p]
        L.orc_depuncture.restype = C.c_int
        L.orc_encode.argtypes = [C.c_int, C.c_int, _u8p, _i32p, _i32p, _i32p, _i32p, _i32p]
        L.orc_encode.restype = C.c_long
        L.orc_demap_c64.argtypes = [_f32p, C.c_long, _f32p, C.c_int, C.c_int, C.c_double, C.c_int, _f64p]
        L.orc_demap_c128.argtypes = [_f64p, C.c_long, _f64p, C.c_int, C.c_int, C.c_double, _f64p]
        L.orc_jac.argtypes = [C.c_float, C.c_float]
        L.orc_jac.restype = C.c_float
        L.orc_lse4.argtypes = [C.c_float] * 4
        L.orc_lse4.restype = C.c_float
        L.orc_set_trans.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        _lib = L
    return _lib


_trans_keep = None


def set_trans(tables=None):
    """Pin the log-MAP primitives E(t) = 2^-t and L(w) = log2(w) to a device's
    exhaustive tables: tables = (etab f32, e_lo_bits, ltab f32, l_lo_bits) as
    captured by modulations_amd.dvb_rcs2_turbo.capture_trans_tables(); None
    restores the correctly rounded primitives."""
    global _trans_keep
    L = lib()
    if tables is None:
        L.orc_set_trans(None, 0, 0, None, 0, 0)
        _trans_keep = None
        return
    et, elo, lt, llo = tables
    et = np.ascontiguousarray(et, np.float32)
    lt = np.ascontiguousarray(lt, np.float32)
    _trans_keep = (et, lt)
    L.orc_set_trans(et.ctypes.data, int(elo), et.size, lt.ctypes.data, int(llo), lt.size)


def trans_pinned():
    """Whether set_trans() currently pins the log-MAP primitives to a device's
    tables (a log-MAP result computed then differs from one computed with the
    correctly rounded primitives: callers that cache results key on this)."""
    return _trans_keep is not None


def trellis():
    t = np.zeros((5, 16, 4), np.int32)
    G = np.zeros((4, 4), np.int32)
    lib().orc_trellis(t, G)
    return t, G


def interleaver(n, params):
    perm = np.zeros(n, np.int32)
    inv = np.zeros(n, np.int32)
    lib().orc_interleaver(n, np.asarray(params, np.int32), perm, inv)
    return perm, inv


def siso(LcA, LcB, LcW, LcY, LaA, LaB, tables, sf, algo=0):
    """bcjr_max_log_map (dvb_rcs2_turbo.py:116-281).  The channel LLRs keep numba's
    typing: four float32 arrays run the f32 specialisation, anything else (float64,
    integers, a mix) the float64 one -- every use widens Lc to f64 first, so the
    values widened exactly give the same results (the product's dispatch rule)."""
    n = len(LcA)
    c = lambda x, dt: np.ascontiguousarray(x, dt)
    LeA = np.zeros(n)
    LeB = np.zeros(n)
    lc = [np.asarray(x) for x in (LcA, LcB, LcW, LcY)]
    if all(x.dtype == np.float32 for x in lc):
        lib().orc_siso(n, *(c(x, np.float32) for x in lc), c(LaA, np.float64), c(LaB, np.float64),
                       c(tables, np.int32), float(sf), algo, LeA, LeB)
    else:
        lib().orc_siso64(n, *(c(x, np.float64) for x in lc), c(LaA, np.float64), c(LaB, np.float64),
                         c(tables, np.int32), float(sf), algo, LeA, LeB)
    return LeA, LeB


def siso_depths(LcA, LcB, LcW, LcY, LaA, LaB, tables, sf, algo=0):
    """Where the reference's second passes meet its first, for the inputs of siso()
    (algo 0 or 1, the same dtype rule): (f2, b2).  f2 is the smallest k in 0..N with
    alpha2[k] == alpha1[k] on all 16 states, b2 the smallest d in 0..N with
    beta2[N-d] == beta1[N-d]; -1: no such step.  C ==, so a NaN never merges."""
    n = len(LcA)
    lc = [np.asarray(x) for x in (LcA, LcB, LcW, LcY)]
    f64 = not all(x.dtype == np.float32 for x in lc)
    lc = [np.ascontiguousarray(x, np.float64 if f64 else np.float32) for x in lc]
    d = np.zeros(2, np.int32)
    rc = lib().orc_siso_depths(n, int(f64), *(x.ctypes.data for x in lc), np.ascontiguousarray(LaA, np.float64),
                               np.ascontiguousarray(LaB, np.float64), np.ascontiguousarray(tables, np.int32),
                               float(sf), algo, d)
    if rc:
        raise ValueError(f"oracle error {rc}")
    return int(d[0]), int(d[1])


def decode_depths(llr, n, period, punct, iterations, perm, inv, tables, algo=0):
    """siso_depths of every SISO call of decode(): int32 [iterations][2][2], indexed
    by SISO 1 / SISO 2 and F2 / B2."""
    llr = np.ascontiguousarray(llr, np.float32)
    d = np.zeros((iterations, 2, 2), np.int32)
    rc = lib().orc_decode_depths(n, period, np.ascontiguousarray(punct, np.uint8), iterations, algo,
                                 np.ascontiguousarray(perm, np.int32), np.ascontiguousarray(inv, np.int32),
                                 np.ascontiguousarray(tables, np.int32), llr, llr.size, d)
    if rc:
        raise IndexError("llr too short") if rc == -1 else ValueError(f"oracle error {rc}")
    return d


def depuncture(llr, n, period, punct):
    """The de-puncture walk of decode() (:476-487): float32 [6][n] planes
    A, B, W1, Y1, W2, Y2, punctured entries zero."""
    llr = np.ascontiguousarray(llr, np.float32)
    out = np.zeros((6, n), np.float32)
    if lib().orc_depuncture(n, period, np.ascontiguousarray(punct, np.uint8), llr, llr.size, out):
        raise IndexError("llr too short")
    return out


def decode(llr, n, period, punct, iterations, perm, inv, tables, algo=0, want_lfinal=False):
    llr = np.ascontiguousarray(llr, np.float32)
    bits = np.zeros(2 * n, np.int32)
    lf = np.zeros(2 * n) if want_lfinal else None
    rc = lib().orc_decode(n, period, np.ascontiguousarray(punct, np.uint8), iterations, algo,
                          np.ascontiguousarray(perm, np.int32), np.ascontiguousarray(inv, np.int32),
                          np.ascontiguousarray(tables, np.int32), llr, llr.size, bits,
                          lf.ctypes.data if lf is not None else None)
    if rc:
        raise IndexError("llr too short") if rc == -1 else ValueError(f"oracle error {rc}")
    return (bits, lf) if want_lfinal else bits


def decode_batch(llr, n, period, punct, iterations, perm, inv, tables, algo=0, nthreads=0,
                 want_lfinal=False):
    llr = np.ascontiguousarray(llr, np.float32)
    B = llr.shape[0]
    bits = np.zeros((B, 2 * n), np.int32)
    lf = np.zeros((B, 2 * n)) if want_lfinal else None
    rc = lib().orc_decode_batch(B, n, period, np.ascontiguousarray(punct, np.uint8), iterations, algo,
                                np.ascontiguousarray(perm, np.int32), np.ascontiguousarray(inv, np.int32),
                                np.ascontiguousarray(tables, np.int32), llr, llr.shape[1], llr.shape[1],
                                bits, lf.ctypes.data if lf is not None else None, nthreads)
    if rc:
        raise ValueError(f"oracle error {rc}")
    return (bits, lf) if want_lfinal else bits


def encode(bits, n, period, punct, perm, tables, G):
    bits = np.ascontiguousarray(bits, np.int32)
    out = np.zeros(6 * n + 8, np.int32)
    m = lib().orc_encode(n, period, np.ascontiguousarray(punct, np.uint8), np.ascontiguousarray(perm, np.int32),
                         np.ascontiguousarray(tables, np.int32), np.ascontiguousarray(G, np.int32), bits, out)
    return out[:m].copy()


def demap(syms, constellation, bps, noise_var, div_f32=False):
    """compute_llr semantics; the arithmetic dtype is numpy's promotion of
    (symbols, constellation).  div_f32: noise_var was a Python float and the
    arithmetic is complex64 (NEP 50 keeps min_d0 - min_d1 in float32)."""
    syms = np.asarray(syms)
    constellation = np.asarray(constellation)
    M = len(constellation)
    out = np.zeros(len(syms) * bps)
    if syms.dtype == np.complex128 or constellation.dtype == np.complex128:
        s = np.ascontiguousarray(syms.astype(np.complex128).view(np.float64))
        cons = np.ascontiguousarray(constellation.astype(np.complex128).view(np.float64))
        lib().orc_demap_c128(s, len(syms), cons, M, bps, float(noise_var), out)
        return out
    s = np.ascontiguousarray(syms.astype(np.complex64).view(np.float32))
    cons = np.ascontiguousarray(constellation.astype(np.complex64).view(np.float32))
    lib().orc_demap_c64(s, len(syms), cons, M, bps, float(noise_var), int(div_f32), out)
    return out


# ---------------------------------------------------------------- modem oracle -------------
# modem_oracle.c: the reference's mappers, hard demods, FIR forms and IQ
# sample format.  Same rule: tests only.
_MSO = os.path.join(_HERE, "liboracle_modem.so")
_mlib = None
_i8p = np.ctypeslib.ndpointer(np.int8, flags="C_CONTIGUOUS")


def mlib():
    global _mlib
    if _mlib is None:
        if not os.path.exists(_MSO):
            build()
        L = C.CDLL(_MSO)
        L.orm_map.argtypes = [_u8p, C.c_long, C.c_int, _f64p, _f64p]
        L.orm_demod_gt0.argtypes = [_f64p, C.c_long, _u8p]
        L.orm_demod_qpsk.argtypes = [_f64p, C.c_long, _u8p]
        L.orm_demod_psk8_f32.argtypes = [_f32p, C.c_long, _i32p, C.c_int, _u8p]
        L.orm_demod_psk8_f32.restype = C.c_long
        L.orm_demod_psk8_f64.argtypes = [_f64p, C.c_long, _i32p, C.c_int, _u8p]
        L.orm_demod_psk8_f64.restype = C.c_long
        L.orm_demod_qam_axis.argtypes = [_f64p, C.c_long, C.c_int, C.c_double, _i32p, _u8p]
        L.orm_demod_qam_axis.restype = C.c_long
        L.orm_demod_argmin.argtypes = [_f64p, C.c_long, C.c_int, _f64p, _u8p]
        L.orm_fir.argtypes = [_f64p, C.c_long, _f64p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, _f64p]
        L.orm_iq_quantize_f64.argtypes = [_f64p, C.c_long, _i8p]
        L.orm_iq_quantize_f32.argtypes = [_f32p, C.c_long, _i8p]
        L.orm_iq_dequantize.argtypes = [_u8p, C.c_long, _f32p]
        _mlib = L
    return _mlib


def _c128(x):
    return np.ascontiguousarray(np.asarray(x).astype(np.complex128).ravel()).view(np.float64)


def modem_map(bits, bps, table):
    bits = np.ascontiguousarray(np.asarray(bits).ravel(), np.uint8)
    n_sym = -(-bits.size // bps)
    out = np.zeros(2 * n_sym)
    mlib().orm_map(bits, bits.size, bps, _c128(table), out)
    return out.view(np.complex128).astype(np.asarray(table).dtype)


def modem_demod(syms, kind, bps, labels=None, scale=0.0, cons=None, nan_raises=True):
    """(bits uint8, nan count) of the rule `kind` (0 GT0, 1 QPSK, 2 PSK8, 3 QAM_AXIS, 4 ARGMIN)."""
    syms = np.asarray(syms).ravel()
    n = syms.size
    out = np.zeros(n * bps, np.uint8)
    L = mlib()
    nans = 0
    if kind == 0:
        L.orm_demod_gt0(_c128(syms), n, out)
    elif kind == 1:
        L.orm_demod_qpsk(_c128(syms), n, out)
    elif kind == 2:
        lab = np.ascontiguousarray(np.arange(8) if labels is None else labels, np.int32)
        if syms.dtype == np.complex64:
            nans = L.orm_demod_psk8_f32(np.ascontiguousarray(syms).view(np.float32), n, lab, int(nan_raises), out)
        else:
            nans = L.orm_demod_psk8_f64(_c128(syms), n, lab, int(nan_raises), out)
    elif kind == 3:
        k = bps // 2
        lab = np.ascontiguousarray(np.arange(1 << k) if labels is None else labels, np.int32)
        nans = L.orm_demod_qam_axis(_c128(syms), n, k, float(scale), lab, out)
    else:
        L.orm_demod_argmin(_c128(syms), n, bps, _c128(cons), out)
    return out, nans


def modem_fir(x, taps, up, down, offset, n_out):
    out = np.zeros(2 * n_out)
    xs = _c128(x)
    h = np.ascontiguousarray(taps, np.float64)
    mlib().orm_fir(xs, xs.size // 2, h, h.size, up, down, offset, n_out, out)
    return out.view(np.complex128)


def modem_iq_quantize(sig):
    sig = np.asarray(sig).ravel()
    out = np.zeros(2 * sig.size, np.int8)
    if sig.dtype == np.complex64:
        mlib().orm_iq_quantize_f32(np.ascontiguousarray(sig).view(np.float32), sig.size, out)
    else:
        mlib().orm_iq_quantize_f64(_c128(sig), sig.size, out)
    return out


def modem_iq_dequantize(raw):
    raw = np.ascontiguousarray(np.asarray(raw, np.uint8).ravel())
    out = np.zeros(2 * (raw.size // 2), np.float32)
    mlib().orm_iq_dequantize(raw, raw.size // 2, out)
    return out.view(np.complex64)
