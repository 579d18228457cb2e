"""numpy restatement of the per-row decision-directed noise variance estimate
(tdec_noise_var_dev; the receiver's rule is
test_sdr_with_coding.py:459-467): the hard decision is the first minimum, in
label order, of dx*dx + dy*dy over the table (f64 differences of the f32 symbol
and the table point), e_s is that minimum, and

    nv[r] = max_py(sum_s e_s / S, floor),   max_py(a, b) = b if b > a else a

which is Python's max(nv, 0.02): a NaN mean stays NaN.  A NaN or infinite symbol
makes its e_s, and so its row's value, NaN.  Everything in float64 (the reference
takes numpy's float32 pairwise mean; the difference is a rounding one)."""
import numpy as np


def sq_errors(syms, cons):
    """e_s of complex64 symbols [..., S] against the label-ordered table."""
    syms = np.asarray(syms)
    assert syms.dtype == np.complex64
    cons = np.asarray(cons)
    sr, si = syms.real.astype(np.float64), syms.imag.astype(np.float64)
    dx = sr[..., None] - cons.real.astype(np.float64)
    dy = si[..., None] - cons.imag.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = dx * dx + dy * dy
        first = np.argmin(d, axis=-1)                      # the first minimum in label order
        e = np.take_along_axis(d, first[..., None], axis=-1)[..., 0]
    return np.where(np.isfinite(sr) & np.isfinite(si), e, np.nan)


def noise_var_rows(syms, cons, floor=0.02):
    """float64 [B]: the estimate of each row of complex64 [B, S] symbols."""
    e = sq_errors(syms, cons)
    mean = e.sum(axis=1) / e.shape[1]
    return np.where(floor > mean, np.float64(floor), mean)   # max_py: a NaN mean stays NaN
