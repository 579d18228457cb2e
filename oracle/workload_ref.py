"""TEST INFRASTRUCTURE ONLY -- host restatement of the counter-based workload
generator (modulations_amd/csrc/tdec_workload.hip) used to check the device
kernels.  Not a reference algorithm: the reference draws its test data with
numpy's global RNG (turbo_test_suite.py:136); the build's generator is
Philox4x32-10 (Salmon et al. SC'11, Random123 philox4x32_R(10)) counted by the
GLOBAL codeword index so data never depends on batching or sharding.  Checked
against Random123's published known-answer vectors in tests/test_workload_host.py.
"""
from __future__ import annotations

import numpy as np

INFO_DOMAIN, NOISE_DOMAIN = 0x1AF0, 0x2B0E
_M = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over broadcastable uint32 counters; returns 4 uint32 arrays."""
    c = [np.asarray(x, np.uint64) & _M for x in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0, k1 = np.uint64(k0) & _M, np.uint64(k1) & _M
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & _M
            k1 = (k1 + np.uint64(0xBB67AE85)) & _M
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M
    return [x.astype(np.uint32) for x in (c0, c1, c2, c3)]


def info_bits(cw_global, n_couples, seed):
    """uint8 [len(cw_global), 2N]: info bit j = bit j%32 of word (j%128)/32 of block j/128."""
    cw = np.asarray(cw_global, np.uint64)[:, None]
    nb = (2 * n_couples + 127) // 128
    blk = np.arange(nb, dtype=np.uint64)[None, :]
    w = philox4x32_10(cw & _M, cw >> np.uint64(32), blk, INFO_DOMAIN, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=-1).reshape(len(cw), nb * 4)             # [cw][block*4 + q]
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(len(cw), nb * 128)[:, :2 * n_couples].astype(np.uint8)


def uniform24(x):
    """The device's Box-Muller uniform of a 32-bit word: ((float)(x >> 8) + 0.5f) * 2^-24 formed
    in float32, returned as float64.  In (0, 1]: from x >> 8 = 2^23 on the + 0.5f is not
    representable and rounds to even, so x >> 8 = 2^24 - 1 gives exactly 1.0."""
    x = np.asarray(x, np.uint32)
    return (((x >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)


def stream_words(cw_global, n, seed, domain):
    """(a, b) uint32 [len(cw), n]: the two words of element s = 0 .. n-1 of a Box-Muller stream,
    philox4x32_10({cw_lo, cw_hi, s >> 1, domain}, seed): words x, y for even s and z, w for odd s."""
    cw = np.asarray(cw_global, np.uint64)[:, None]
    s = np.arange(n, dtype=np.uint64)[None, :]
    r = philox4x32_10(cw & _M, cw >> np.uint64(32), s >> np.uint64(1), domain, seed & 0xFFFFFFFF, seed >> 32)
    odd = np.broadcast_to((s & np.uint64(1)).astype(bool), r[0].shape)
    return np.where(odd, r[2], r[0]), np.where(odd, r[3], r[1])


def sincospi(t):
    """(sin(pi t), cos(pi t)) in float64, exact at the multiples of 1/2 as sincospi is: t is
    split into the nearest multiple of 1/2 and a remainder of at most 1/4 (both exact)."""
    t = np.asarray(t, np.float64)
    k = np.rint(2.0 * t)
    d = np.pi * (t - 0.5 * k)
    s, c = np.sin(d), np.cos(d)
    q = k.astype(np.int64) & 3
    return (np.choose(q, [s, c, -s, -c]) + 0.0), (np.choose(q, [c, -s, -c, s]) + 0.0)   # + 0.0: no -0.0


def box_muller(a, b, sigma):
    """complex128 Box-Muller of the words (a, b): the float32 uniforms of uniform24, everything
    behind them in float64; sigma is rounded to float32 first, as the device holds it.
    u1 = 1 gives radius 0 and u2 = 1 the angle 2 pi: (radius, 0) exactly."""
    u1, u2 = uniform24(a), uniform24(b)
    rad = np.float64(np.float32(sigma)) * np.sqrt(-2.0 * np.log(u1) + 0.0)
    sn, cs = sincospi(2.0 * u2)
    return rad * cs + 1j * (rad * sn)


def awgn(cw_global, n_sym, seed, sigma, branch=0):
    """complex [len(cw), n_sym] noise of receive branch `branch`: Box-Muller in float64 of the
    device's float32 uniforms and float32 sigma (the device goes on in f32)."""
    return box_muller(*stream_words(cw_global, n_sym, seed, NOISE_DOMAIN | (branch << 16)), sigma)
