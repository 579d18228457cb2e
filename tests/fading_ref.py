"""Flat fading: numpy restatements of the equaliser
(k_equalize, tdec_equalize_dev) and of the generator's gain draw
(tdec_workload_fading_dev).

TEST INFRASTRUCTURE.  The equaliser is build-defined and stated so that this float64
restatement matches it bit for bit: the products of float32 values are exact in
float64, so every sum, quotient and the final cast to float32 rounds once, on the
device as here.  The gain draw is the device's Box-Muller in float64 of the device's
float32 uniforms (the device goes on in float32), as oracle/workload_ref.py restates the noise.
"""
import numpy as np

from oracle.workload_ref import box_muller, stream_words

FADE_DOMAIN = 0x3C5D


def equalize(y, h, nv, coh=1):
    """y complex64 [B, S], h complex64 [B, ceil(S / coh)], nv a scalar or float64 [B]
    -> (z complex64 [B, S], nv_sym float64 [B, S]).  Symbol s uses h[:, s // coh];
    |h|^2 zero or not finite is an erasure: z = 0, nv_sym = +inf."""
    y = np.asarray(y, np.complex64)
    h = np.asarray(h, np.complex64)
    B, S = y.shape
    hs = h[:, np.arange(S) // coh]
    hr, hi = hs.real.astype(np.float64), hs.imag.astype(np.float64)
    yr, yi = y.real.astype(np.float64), y.imag.astype(np.float64)
    nv = np.broadcast_to(np.asarray(nv, np.float64).reshape(-1, 1), (B, 1)) if np.ndim(nv) else np.float64(nv)
    with np.errstate(all="ignore"):
        g = hr * hr + hi * hi
        zr = ((yr * hr + yi * hi) / g).astype(np.float32)
        zi = ((yi * hr - yr * hi) / g).astype(np.float32)
        nvs = nv / g
    erased = (g == 0) | ~np.isfinite(g)
    z = np.empty((B, S), np.complex64)
    z.real = np.where(erased, np.float32(0), zr)
    z.imag = np.where(erased, np.float32(0), zi)
    return z, np.where(erased, np.inf, nvs)


def los_scat(K):
    """(los, scat) = (sqrt(K / (K + 1)), sqrt(1 / (K + 1))) rounded to float32, as the device
    holds them, returned as float64."""
    K = np.float64(K)
    return np.float64(np.float32(np.sqrt(K / (K + 1.0)))), np.float64(np.float32(np.sqrt(1.0 / (K + 1.0))))


def gains(cw_global, n_blocks, seed, K=0.0, branch=0):
    """complex128 [len(cw_global), n_blocks]: h = sqrt(K / (K + 1)) + sqrt(1 / (K + 1)) w,
    w ~ CN(0, 1) by Box-Muller on philox4x32_10({g_lo, g_hi, j / 2, FADE_DOMAIN | branch << 16},
    seed) for gain block j of global codeword g (words x, y for even j, z, w for odd j), the
    noise stream's uniform mapping: oracle.workload_ref.box_muller with sigma = sqrt(1/2)."""
    w = box_muller(*stream_words(cw_global, n_blocks, seed, FADE_DOMAIN | (branch << 16)), np.sqrt(0.5))
    los, scat = los_scat(K)
    return los + scat * w


def demap_per_symbol(z, cons, bps, nv_sym, div_f32):
    """oracle.demap of every symbol of z [B, S] with its own noise variance: float64
    [B, S * bps], reference sign.  One oracle call per distinct value."""
    from oracle import oracle as O
    z = np.asarray(z)
    B, S = z.shape
    out = np.zeros((B, S, bps))
    flat_nv = np.asarray(nv_sym, np.float64).reshape(-1)
    keys = flat_nv.view(np.int64)
    for k in np.unique(keys):
        idx = np.flatnonzero(keys == k)
        llr = O.demap(z.reshape(-1)[idx], cons, bps, float(flat_nv[idx[0]]), div_f32)
        out.reshape(-1, bps)[idx] = llr.reshape(-1, bps)
    return out.reshape(B, S * bps)
