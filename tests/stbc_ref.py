"""Transmit diversity (include/stbc.h): numpy restatements of the Alamouti
combiner (k_stbc_combine, stbc_combine_dev), of the transmit mapping and of the generator's
2 x R link (stbc_workload_dev).

TEST INFRASTRUCTURE.  The combiner is build-defined and stated so that this float64 restatement
matches it bit for bit: the products of float32 values are exact in float64, and every sum,
difference, quotient and the final cast to float32 rounds once, on the device as here.  The four
products of a part are added in the header's order -- the two inner additions, then the outer one
-- and the sums over the branches are plain loops over r = 0 .. R-1 (np.sum adds pairwise: another
order, other roundings).  The generator's signal is the header's float32 expression stepped in
float32; its gains and noise are the float64 references of tests/generator_cases.py, antenna 1's
gains on the domain word 0x6F8A.
"""
import numpy as np

import fading_ref as F
import generator_cases as GC
from oracle import workload_ref as W

F32, F64 = np.float32, np.float64
FADE1_DOMAIN = 0x6F8A                              # antenna 1's gains; antenna 0's: fading_ref.FADE_DOMAIN
SQRT_HALF = F32(0.70710678118654752)               # raw gain -> effective gain, per component in float32


def s2_of(S):
    return S + (S & 1)


def combine(y, h, nv, S=None, coh=2):
    """y complex64 [B, R, S2], h complex64 [B, R, 2, ceil(S2 / coh)], nv a scalar, float64 [B]
    (common to a burst's branches) or float64 [B, R] (per branch) -> (z complex64 [B, S], nv_sym
    float64 [B, S]); S defaults to S2, an odd S = S2 - 1 drops the pad slot's second output.
    A branch whose |h0|^2 + |h1|^2 is zero or not finite is skipped; each sum starts from the
    first live branch's term; no live branch, or a zero or infinite G, is an erasure (z = 0,
    nv_sym = +inf); a NaN sum stays NaN."""
    y, h = np.asarray(y, np.complex64), np.asarray(h, np.complex64)
    B, R, S2 = y.shape
    assert S2 % 2 == 0 and coh >= 2 and coh % 2 == 0
    S = S2 if S is None else S
    assert S in (S2, S2 - 1)
    P = S2 // 2
    per_branch = np.ndim(nv) == 2
    nv = np.asarray(nv, F64)
    blk = (2 * np.arange(P)) // coh
    G, ar, ai, br, bi = (np.zeros((B, P)) for _ in range(5))
    live = np.zeros((B, P), bool)
    with np.errstate(all="ignore"):
        for r in range(R):
            h0, h1 = h[:, r, 0][:, blk], h[:, r, 1][:, blk]
            y0, y1 = y[:, r, 0::2], y[:, r, 1::2]
            h0r, h0i, h1r, h1i = (v.astype(F64) for v in (h0.real, h0.imag, h1.real, h1.imag))
            y0r, y0i, y1r, y1i = (v.astype(F64) for v in (y0.real, y0.imag, y1.real, y1.imag))
            g = (h0r * h0r + h0i * h0i) + (h1r * h1r + h1i * h1i)
            t = [(y0r * h0r + y0i * h0i) + (y1r * h1r + y1i * h1i),
                 (y0i * h0r - y0r * h0i) + (y1r * h1i - y1i * h1r),
                 (y0r * h1r + y0i * h1i) - (y1r * h0r + y1i * h0i),
                 (y0i * h1r - y0r * h1i) - (y1r * h0i - y1i * h0r)]
            ok = ~((g == 0) | ~np.isfinite(g))
            if per_branch:
                w = nv[:, r][:, None]
                g, t = g / w, [v / w for v in t]
            first, later = ok & ~live, ok & live
            G = np.where(first, g, np.where(later, G + g, G))
            ar, ai, br, bi = (np.where(first, v, np.where(later, acc + v, acc)) for acc, v in zip((ar, ai, br, bi), t))
            live |= ok
        q = [(v / G).astype(F32) for v in (ar, ai, br, bi)]
        top = F64(1.0) if per_branch else (nv.reshape(-1, 1) if nv.ndim else nv)
        nvp = top / G
    erased = ~live | (G == 0) | np.isinf(G)
    q = [np.where(erased, F32(0), v) for v in q]
    nvp = np.where(erased, np.inf, nvp)
    z = np.empty((B, S2), np.complex64)
    z.real[:, 0::2], z.imag[:, 0::2], z.real[:, 1::2], z.imag[:, 1::2] = q
    return np.ascontiguousarray(z[:, :S]), np.ascontiguousarray(np.repeat(nvp, 2, axis=1)[:, :S])


def transmit(x):
    """The transmit mapping: table points x complex64 [..., S] -> (antenna 0's slots, antenna 1's slots),
    complex64 [..., S2] each: slot 2m sends (x[2m], x[2m+1]), slot 2m+1 (-conj(x[2m+1]), conj(x[2m])); the
    pad point of an odd S is 0 + 0j."""
    x = np.asarray(x, np.complex64)
    S = x.shape[-1]
    xp = np.zeros((*x.shape[:-1], s2_of(S)), np.complex64)
    xp[..., :S] = x
    a0, a1 = np.empty_like(xp), np.empty_like(xp)
    a0[..., 0::2], a1[..., 0::2] = xp[..., 0::2], xp[..., 1::2]
    a0[..., 1::2] = GC.to_c64(-xp[..., 1::2].real, xp[..., 1::2].imag)
    a1[..., 1::2] = GC.to_c64(xp[..., 0::2].real, -xp[..., 0::2].imag)
    return a0, a1


def signal32(h, x, coh):
    """The generator's noise-free slots, complex64 [B, R, S2], of the written gains h complex64
    [B, R, 2, nh] and the table points x complex64 [B, S]: h0 s0 + h1 s1 stepped in float32 in the
    header's order, re = (h0r s0r - h0i s0i) + (h1r s1r - h1i s1i), im = (h0r s0i + h0i s0r) +
    (h1r s1i + h1i s1r)."""
    h = np.asarray(h, np.complex64)
    a0, a1 = transmit(x)
    blk = np.arange(a0.shape[-1]) // coh
    h0, h1 = h[:, :, 0][:, :, blk], h[:, :, 1][:, :, blk]
    s0, s1 = a0[:, None, :], a1[:, None, :]
    re = (h0.real * s0.real - h0.imag * s0.imag) + (h1.real * s1.real - h1.imag * s1.imag)
    im = (h0.real * s0.imag + h0.imag * s0.real) + (h1.real * s1.imag + h1.imag * s1.real)
    assert re.dtype == F32 and im.dtype == F32
    return GC.to_c64(re, im)


def raw_gains(cw_global, R, n_blocks, seed, K, antenna):
    """(raw gains complex128 [n, R, n_blocks], the tolerance's radius scat * rad): antenna 0's are
    generator_cases.gains (the branch generator's draw), antenna 1's the same draw on FADE1_DOMAIN."""
    if antenna == 0:
        pairs = [GC.gains(cw_global, n_blocks, seed, K, b) for b in range(R)]
    else:
        los, scat = F.los_scat(K)
        pairs = []
        for b in range(R):
            a, c = W.stream_words(cw_global, n_blocks, seed, FADE1_DOMAIN | (b << 16))
            pairs.append((los + scat * W.box_muller(a, c, np.sqrt(0.5)), scat * GC.radius(a, GC.SQRT_HALF)))
    return np.stack([p[0] for p in pairs], axis=1), np.stack([p[1] for p in pairs], axis=1)


def gains(cw_global, R, n_blocks, seed, K=0.0):
    """(effective gains complex128 [n, R, 2, n_blocks], their radius): float64(SQRT_HALF) times raw_gains."""
    g0, r0 = raw_gains(cw_global, R, n_blocks, seed, K, 0)
    g1, r1 = raw_gains(cw_global, R, n_blocks, seed, K, 1)
    c = F64(SQRT_HALF)
    return c * np.stack([g0, g1], axis=2), c * np.stack([r0, r1], axis=2)


def gains_excess(dev, ref, rad):
    """generator_cases.excess for an effective gain, per component: what is over the roundings, over the
    radius, to compare with generator_cases.bound().  The raw gain is inside that module's tolerance,
    ulp32(raw) / 2 + bound rad_raw; the product with c = SQRT_HALF scales this by c and rounds once more,
    ulp32(c raw) / 2.  c raw lies one binade below raw or in the same one, so ulp32(raw) <= 2 ulp32(c raw) and
    c ulp32(raw) / 2 <= c ulp32(c raw): the roundings' share is at most (1/2 + c) ulp32 of the effective
    gain, and the rest is bound * (c rad_raw) = bound * rad."""
    dev, ref = np.asarray(dev), np.asarray(ref, np.complex128)
    out = []
    for d, y in ((dev.real, ref.real), (dev.imag, ref.imag)):
        slack = (0.5 + F64(SQRT_HALF)) * np.spacing(np.abs(y).astype(F32)).astype(F64)
        over = np.maximum(np.abs(d.astype(F64) - y) - slack, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(over == 0.0, 0.0, np.where(rad > 0, over / rad, np.inf)))
    return np.stack(out)


def noise(cw_global, R, n_slots, seed, sigma):
    """(noise complex128 [n, R, n_slots], radius): branch b's noise stream (generator_cases.noise), slot s
    the sample the branch generator adds at symbol s."""
    pairs = [GC.noise(cw_global, n_slots, seed, sigma, branch=b) for b in range(R)]
    return np.stack([p[0] for p in pairs], axis=1), np.stack([p[1] for p in pairs], axis=1)
