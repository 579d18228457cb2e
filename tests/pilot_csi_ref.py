"""Pilot-aided channel estimation: numpy restatements of the framed
layout, the estimator (k_csi_pilots, tdec_csi_pilots_dev) and the framing generator's
deterministic parts (tdec_workload_frame_dev).

TEST INFRASTRUCTURE.  The estimator is build-defined and stated so that this float64
restatement matches it bit for bit: every sum runs in the order the definition gives (over
a block's pilots in turn, over a row's blocks in turn), numpy neither contracts a multiply
and an add nor reorders an explicit loop, and the products of float32 values are exact in
float64.  The loops run over pilots and blocks; rows are the vector axis.  The equaliser
behind it is tests/fading_ref.py's.
"""
import numpy as np

import fading_ref as F
from oracle.workload_ref import box_muller, philox4x32_10, stream_words

PILOT_DOMAIN = 0x4D6C
CFO_DOMAIN = 0x5E7B
_M = np.uint64(0xFFFFFFFF)


# ---- layout ---------------------------------------------------------------------------------
def n_segments(S, dlen):
    return -(-S // dlen)


def frame_len(S, plen, dlen):
    return S + (n_segments(S, dlen) + 1) * plen


def segment_len(S, dlen, j):
    return min(dlen, S - j * dlen)


def block_start(S, plen, dlen, j):
    J = n_segments(S, dlen)
    return j * (plen + dlen) if j < J else S + J * plen


def data_positions(S, plen, dlen):
    s = np.arange(S)
    return s + (s // dlen + 1) * plen


def default_pilots(n):
    """Pilot k (over the frame's pilots alone) is 1j ** ((k (k + 1) / 2) mod 4)."""
    q = np.array([(k * (k + 1) // 2) % 4 for k in range(n)])
    p = np.empty(n, np.complex64)
    p.real = np.array([1, 0, -1, 0], np.float32)[q]
    p.imag = np.array([0, 1, 0, -1], np.float32)[q]
    return p


# ---- estimator ------------------------------------------------------------------------------
def block_gains(frames, pilots, S, plen, dlen, residuals=False):
    """hp complex128 [B, J + 1] (and q float64 [B, J + 1]): the definition's loops."""
    frames = np.asarray(frames, np.complex64)
    B = frames.shape[0]
    nb = n_segments(S, dlen) + 1
    hr, hi, q = np.empty((B, nb)), np.empty((B, nb)), np.empty((B, nb))
    with np.errstate(all="ignore"):
        for j in range(nb):
            t0 = block_start(S, plen, dlen, j)
            y = frames[:, t0:t0 + plen]
            yr, yi = y.real.astype(np.float64), y.imag.astype(np.float64)
            p = pilots[j * plen:(j + 1) * plen]
            pr, pi = p.real.astype(np.float64), p.imag.astype(np.float64)
            nr, ni, e = np.zeros(B), np.zeros(B), 0.0
            for i in range(plen):
                nr = nr + (yr[:, i] * pr[i] + yi[:, i] * pi[i])
                ni = ni + (yi[:, i] * pr[i] - yr[:, i] * pi[i])
                e = e + (pr[i] * pr[i] + pi[i] * pi[i])
            hr[:, j], hi[:, j] = nr / e, ni / e
            qq = np.zeros(B)
            for i in range(plen):
                dr = yr[:, i] - (hr[:, j] * pr[i] - hi[:, j] * pi[i])
                di = yi[:, i] - (hr[:, j] * pi[i] + hi[:, j] * pr[i])
                qq = qq + (dr * dr + di * di)
            q[:, j] = qq
    hp = np.empty((B, nb), np.complex128)
    hp.real, hp.imag = hr, hi
    return (hp, q) if residuals else hp


def noise_var(q, plen, floor):
    """nv [B] = max_py((q_0 + q_1 + ...) / ((J + 1)(plen - 1)), floor); a NaN stays NaN."""
    with np.errstate(all="ignore"):
        total = q[:, 0].copy()
        for j in range(1, q.shape[1]):
            total = total + q[:, j]
        mean = total / np.float64(q.shape[1] * (plen - 1))
    return np.where(floor > mean, np.float64(floor), mean)


def interpolate(hp, S, plen, dlen, mode="linear"):
    """h complex64 [B, S] from hp complex128 [B, J + 1]."""
    B = hp.shape[0]
    s = np.arange(S)
    j = s // dlen
    u = s - j * dlen
    L = np.minimum(dlen, S - j * dlen)
    w = (2 * u + plen + 1).astype(np.float64) / (2 * (plen + L)).astype(np.float64)
    if mode == "mean":
        w = np.full(S, 0.5)
    a, b = hp[:, j], hp[:, j + 1]
    with np.errstate(all="ignore"):
        re = (a.real + w * (b.real - a.real)).astype(np.float32)
        im = (a.imag + w * (b.imag - a.imag)).astype(np.float32)
    dead = ((a.real == 0) & (a.imag == 0)) | ((b.real == 0) & (b.imag == 0))
    h = np.empty((B, S), np.complex64)
    h.real = np.where(dead, np.float32(0), re)
    h.imag = np.where(dead, np.float32(0), im)
    return h


def estimate(frames, pilots, S, plen, dlen, mode="linear", nv=None, floor=0.02):
    """The whole launch: {"z", "nv_sym", "h", "y", "hp", "nv" (the estimate, plen >= 2; else
    None)}.  nv: a scalar, float64 [B], or None (the estimate equalises)."""
    frames = np.asarray(frames, np.complex64)
    hp, q = block_gains(frames, pilots, S, plen, dlen, residuals=True)
    est = noise_var(q, plen, floor) if plen >= 2 else None
    h = interpolate(hp, S, plen, dlen, mode)
    y = np.ascontiguousarray(frames[:, data_positions(S, plen, dlen)])
    use = est if nv is None else nv
    z, nvs = F.equalize(y, h, use, 1)
    return {"z": z, "nv_sym": nvs, "h": h, "y": y, "hp": hp, "nv": est}


# ---- generator ------------------------------------------------------------------------------
def cfo_of(cw_global, seed, cfo_max):
    """f_g float64 [n]: cfo_max (2u - 1), u = ((x >> 8) + 0.5) 2^-24 of word x of
    philox4x32_10({g_lo, g_hi, 0, CFO_DOMAIN}, seed): the device's own f64 expression."""
    cw = np.asarray(cw_global, np.uint64)
    z = np.zeros_like(cw)
    r = philox4x32_10(cw & _M, cw >> np.uint64(32), z, CFO_DOMAIN, seed & 0xFFFFFFFF, seed >> 32)
    u = ((r[0] >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    return np.float64(cfo_max) * (2.0 * u - 1.0)


def pilot_noise(cw_global, n_pilots, seed, sigma, branch=0):
    """complex128 [n, n_pilots]: the noise of pilot k (over the frame's pilots alone) of receive
    branch `branch`, Box-Muller in oracle.workload_ref.awgn's form on a stream of its own,
    philox4x32_10({g_lo, g_hi, k >> 1, PILOT_DOMAIN | branch << 16}, seed): words x, y for even
    k and z, w for odd k."""
    return box_muller(*stream_words(cw_global, n_pilots, seed, PILOT_DOMAIN | (branch << 16)), sigma)


def rotate(frames0, f_g):
    """Frames of a cfo = 0 run rotated by exp(j 2 pi f_g t), float64 then float32."""
    frames0 = np.asarray(frames0, np.complex64)
    t = np.arange(frames0.shape[1], dtype=np.float64)
    ang = np.pi * (2.0 * (f_g[:, None] * t[None, :]))
    cs, sn = np.cos(ang), np.sin(ang)
    vr, vi = frames0.real.astype(np.float64), frames0.imag.astype(np.float64)
    out = np.empty(frames0.shape, np.complex64)
    out.real = (vr * cs - vi * sn).astype(np.float32)
    out.imag = (vr * sn + vi * cs).astype(np.float32)
    return out
