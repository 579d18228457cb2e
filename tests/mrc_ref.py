"""Receive diversity: numpy restatements of the maximal-ratio
combiner (k_combine, tdec_combine_dev) and of the generator's per-branch gain draw
(tdec_workload_branches_dev).

TEST INFRASTRUCTURE.  The combiner is build-defined and stated so that this float64
restatement matches it bit for bit: the products of float32 values are exact in float64,
and every sum, quotient and the final cast to float32 rounds once, on the device as here.
The sums over the branches are plain loops over r = 0 .. R-1, the definition's order
(np.sum adds pairwise: another order, other roundings).
"""
import numpy as np

import fading_ref as F


def combine(y, h, nv, coh=1):
    """y complex64 [B, R, S], h complex64 [B, R, ceil(S / coh)], nv a scalar, float64 [B]
    (common to a burst's branches) or float64 [B, R] (per branch) -> (z complex64 [B, S],
    nv_sym float64 [B, S]).  A branch whose |h|^2 is zero or not finite is skipped; each
    sum starts from the first live branch's term; no live branch, or a zero or infinite
    sum of weights, is an erasure (z = 0, nv_sym = +inf); a NaN sum stays NaN."""
    y = np.asarray(y, np.complex64)
    h = np.asarray(h, np.complex64)
    B, R, S = y.shape
    per_branch = np.ndim(nv) == 2
    nv = np.asarray(nv, np.float64)
    hs = h[:, :, np.arange(S) // coh]
    G, A, Bm = np.zeros((B, S)), np.zeros((B, S)), np.zeros((B, S))
    live = np.zeros((B, S), bool)
    with np.errstate(all="ignore"):
        for r in range(R):
            hr, hi = hs[:, r].real.astype(np.float64), hs[:, r].imag.astype(np.float64)
            yr, yi = y[:, r].real.astype(np.float64), y[:, r].imag.astype(np.float64)
            g = hr * hr + hi * hi
            a = yr * hr + yi * hi
            b = yi * hr - yr * hi
            ok = ~((g == 0) | ~np.isfinite(g))
            if per_branch:
                w = nv[:, r][:, None]
                g, a, b = g / w, a / w, b / w
            first, later = ok & ~live, ok & live
            G = np.where(first, g, np.where(later, G + g, G))
            A = np.where(first, a, np.where(later, A + a, A))
            Bm = np.where(first, b, np.where(later, Bm + b, Bm))
            live |= ok
        zr, zi = (A / G).astype(np.float32), (Bm / G).astype(np.float32)
        top = np.float64(1.0) if per_branch else (nv.reshape(-1, 1) if nv.ndim else nv)
        nvs = top / G
    erased = ~live | (G == 0) | np.isinf(G)
    z = np.empty((B, S), np.complex64)
    z.real = np.where(erased, np.float32(0), zr)
    z.imag = np.where(erased, np.float32(0), zi)
    return z, np.where(erased, np.inf, nvs)


def gains(cw_global, R, n_blocks, seed, K=0.0):
    """complex128 [len(cw_global), R, n_blocks]: fading_ref.gains with branch b's draw on
    the domain word FADE_DOMAIN | b << 16 (branch 0: fading_ref.gains itself)."""
    return np.stack([F.gains(cw_global, n_blocks, seed, K, branch=b) for b in range(R)], axis=1)
