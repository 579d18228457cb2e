"""The log-MAP (exact log-sum) soft demapper's definition in numpy float64
(DESIGN.md section 9), the reference of the log-MAP demapper tests:

    d_i   = |s - c_i|^2                         over all M points, label i = bits MSB first
    L_b,v = log sum_{i : bit_b(i) = v} exp(-d_i / nv),   nv = max(noise_var, 0.005)
    llr_b = sign * clip(L_b,1 - L_b,0, -30, +30)

evaluated stably (the smallest d_i / nv subtracted before exponentiating), no
cut-off.  Symbols and table are taken as the device sees them: f32 values
widened exactly (or f64 values as they are)."""
import numpy as np

NV_FLOOR = 0.005
CLIP = 30.0


def label_bits(M, bps):
    """bool [M, bps]: bit b (MSB first) of label i."""
    return ((np.arange(M)[:, None] >> (bps - 1 - np.arange(bps))[None, :]) & 1).astype(bool)


def _wide(z):
    z = np.asarray(z)
    return z.real.astype(np.float64), z.imag.astype(np.float64)


def distances(syms, cons):
    """float64 [n_sym, M] squared distances."""
    sr, si = _wide(syms)
    cr, ci = _wide(cons)
    dx = sr[:, None] - cr[None, :]
    dy = si[:, None] - ci[None, :]
    return dx * dx + dy * dy


def raw_llr(syms, cons, bps, noise_var):
    """L_b,1 - L_b,0 before the clip, reference sign: float64 [n_sym, bps],
    and the symbols' d_min [n_sym]."""
    nv = max(float(noise_var), NV_FLOOR)
    d = distances(syms, cons)
    bits = label_bits(len(np.asarray(cons)), bps)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = d / nv
        xm = x.min(axis=1, keepdims=True)
        e = np.exp(-(x - xm))                                 # the shift cancels in L_1 - L_0
        s1 = e @ bits.astype(np.float64)
        s0 = e @ (~bits).astype(np.float64)
        return np.log(s1) - np.log(s0), d.min(axis=1)


def llr(syms, cons, bps, noise_var, sign=+1):
    """float64 [n_sym * bps], the definition."""
    r, _ = raw_llr(syms, cons, bps, noise_var)
    out = np.where(np.isnan(r), r, np.clip(r, -CLIP, CLIP))
    return (sign * out).reshape(-1)


def maxlog_llr(syms, cons, bps, noise_var, sign=+1):
    """The max-log approximation of the same formula in float64 (same nv, clip, sign)."""
    nv = max(float(noise_var), NV_FLOOR)
    d = distances(syms, cons)
    bits = label_bits(len(np.asarray(cons)), bps)
    out = np.empty((d.shape[0], bps))
    for b in range(bps):
        out[:, b] = (d[:, ~bits[:, b]].min(axis=1) - d[:, bits[:, b]].min(axis=1)) / nv
    return (sign * np.clip(out, -CLIP, CLIP)).reshape(-1)
