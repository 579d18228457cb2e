"""Spatial multiplexing (include/sm.h): numpy restatements of the 2 x R
joint max-log detector (k_sm_detect, sm_detect_dev), of the transmit mapping and of the
generator's multiplexed 2 x R link (sm_workload_dev).

TEST INFRASTRUCTURE.  The detector is build-defined and stated so that this float64 restatement
matches it bit for bit: every product, difference, sum and quotient of the header is one rounded
float64 operation here as on the device, in the header's order, with explicit loops over the
branches r and the hypotheses (a, b) -- no np.sum (it adds pairwise: another order) and no complex
multiply (numpy's may fuse or reorder its four products).  Only rows and slots are vectorised.
A minimum's operand order is free: D is never -0 and never NaN.  The generator's signal is the
header's float32 expression stepped in float32; its gains and noise are those of
tests/stbc_ref.py (the Alamouti link's domain words), the noise of slot m the branch generator's
sample at symbol index m.
"""
import numpy as np

import generator_cases as GC
import stbc_ref as SR

F32, F64 = np.float32, np.float64
FLOOR = 0.005                                       # the reference demapper's noise floor


def slots_of(S):
    return (S + 1) // 2


def _nve(nv):
    nv = np.asarray(nv, F64)
    with np.errstate(invalid="ignore"):
        return np.where(nv > FLOOR, nv, FLOOR)      # a NaN takes the floor


def detect(y, h, cons, nv, S=None, coh=1, sign=+1, minima=False):
    """y complex64 [B, R, T], h complex64 [B, R, 2, ceil(T / coh)], cons the label-ordered table
    (M points, widened to float64), nv a scalar, float64 [B] (common to a burst's branches) or
    float64 [B, R] (per branch) -> float32 [B, S * bps]; S defaults to 2 T, an odd S = 2 T - 1
    makes the last slot single-stream.  minima=True: (LLRs, the float64 minima [4][bps][B, T]: stream 0's
    m0 and m1, stream 1's m0 and m1, per bit j and slot), for the tests' error bounds."""
    y, h = np.asarray(y, np.complex64), np.asarray(h, np.complex64)
    cons = np.asarray(cons)
    B, R, T = y.shape
    M = len(cons)
    bps = M.bit_length() - 1
    assert 1 << bps == M and 2 <= M <= 64 and coh >= 1 and 1 <= R <= 8
    S = 2 * T if S is None else S
    assert S in (2 * T, 2 * T - 1)
    cr, ci = cons.real.astype(F64), cons.imag.astype(F64)
    per_branch = np.ndim(nv) == 2
    nve = _nve(nv)
    blk = np.arange(T) // coh
    two = (2 * np.arange(T) + 1 < S)[None, :]       # antenna 1 sends in this slot
    f = lambda v: v.astype(F64)  # noqa: E731
    yr, yi = f(y.real), f(y.imag)
    hs = h[:, :, :, blk]                            # [B, R, 2, T]
    h0r, h0i, h1r, h1i = f(hs[:, :, 0].real), f(hs[:, :, 0].imag), f(hs[:, :, 1].real), f(hs[:, :, 1].imag)
    ok = np.isfinite(yr) & np.isfinite(yi) & np.isfinite(h0r) & np.isfinite(h0i) & np.isfinite(h1r) & np.isfinite(h1i)
    any_live = ok.any(axis=1)                       # [B, T]
    inf = np.full((B, T), np.inf)
    m = np.stack([np.stack([inf] * bps)] * 4)       # [stream 0: m0, m1; stream 1: m0, m1][bit j][B, T]
    with np.errstate(all="ignore"):
        for a in range(M):
            u = [(yr[:, r] - (h0r[:, r] * cr[a] - h0i[:, r] * ci[a]), yi[:, r] - (h0r[:, r] * ci[a] + h0i[:, r] * cr[a]))
                 for r in range(R)]
            for b in range(M):
                D = np.zeros((B, T))
                live = np.zeros((B, T), bool)
                for r in range(R):
                    ure, uim = u[r]
                    vre = np.where(two, ure - (h1r[:, r] * cr[b] - h1i[:, r] * ci[b]), ure)
                    vim = np.where(two, uim - (h1r[:, r] * ci[b] + h1i[:, r] * cr[b]), uim)
                    d = vre * vre + vim * vim
                    if per_branch:
                        d = d / nve[:, r][:, None]
                    o = ok[:, r]
                    D = np.where(o & ~live, d, np.where(o & live, D + d, D))   # from the first live term
                    live |= o
                for j in range(bps):
                    ka, kb = (a >> (bps - 1 - j)) & 1, 2 + ((b >> (bps - 1 - j)) & 1)
                    m[ka, j] = np.minimum(m[ka, j], D)
                    m[kb, j] = np.minimum(m[kb, j], D)
        out = np.zeros((B, T, 2, bps), F32)
        for s in (0, 1):
            for j in range(bps):
                l = m[2 * s, j] - m[2 * s + 1, j]
                if not per_branch:
                    l = l / (nve.reshape(-1, 1) if nve.ndim else nve)
                v = F32(sign) * np.clip(l, -30.0, 30.0).astype(F32)
                out[:, :, s, j] = np.where(any_live & ~np.isnan(l), v, F32(0.0))
    out = np.ascontiguousarray(out.reshape(B, 2 * T * bps)[:, :S * bps])
    return (out, m) if minima else out


def transmit(x):
    """The transmit mapping: table points x complex64 [..., S] -> (antenna 0's slots, antenna 1's
    slots), complex64 [..., T] each: slot m sends (x[2m], x[2m+1]); the silent antenna of an odd
    S sends 0 + 0j."""
    x = np.asarray(x, np.complex64)
    S = x.shape[-1]
    xp = np.zeros((*x.shape[:-1], 2 * slots_of(S)), np.complex64)
    xp[..., :S] = x
    return np.ascontiguousarray(xp[..., 0::2]), np.ascontiguousarray(xp[..., 1::2])


def signal32(h, x, coh):
    """The generator's noise-free slots, complex64 [B, R, T], of the written gains h complex64
    [B, R, 2, nh] and the table points x complex64 [B, S]: h0 s0 + h1 s1 stepped in float32 in the
    header's order."""
    h = np.asarray(h, np.complex64)
    a0, a1 = transmit(x)
    blk = np.arange(a0.shape[-1]) // coh
    h0, h1 = h[:, :, 0][:, :, blk], h[:, :, 1][:, :, blk]
    s0, s1 = a0[:, None, :], a1[:, None, :]
    re = (h0.real * s0.real - h0.imag * s0.imag) + (h1.real * s1.real - h1.imag * s1.imag)
    im = (h0.real * s0.imag + h0.imag * s0.real) + (h1.real * s1.imag + h1.imag * s1.real)
    assert re.dtype == F32 and im.dtype == F32
    return GC.to_c64(re, im)


# the gains are the Alamouti link's (stbc_ref.gains: antenna 0 the branch generator's draw, antenna 1 the
# same draw on 0x6F8A, both times float32 sqrt(1/2)), block j covering slots [j coh, (j + 1) coh); the
# noise of slot m is branch b's sample at symbol index m
gains, gains_excess, noise, SQRT_HALF = SR.gains, SR.gains_excess, SR.noise, SR.SQRT_HALF
