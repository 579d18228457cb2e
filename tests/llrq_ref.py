"""numpy restatement of the quantised LLR definitions (include/llrq.h).

quantize        q = int8(clip(rint(float32(x) * inv_step), -127, 127)), inv_step = float32(1) / step:
                one float32 multiply, round to nearest with ties to even; NaN -> 0, +-inf -> +-127,
                -0.0 -> 0.  A float64 input is rounded to float32 first.
saturated       how many elements have |float32(x) * inv_step| > 127 (the infinities included).
dequantize_i8   float32(q) * step, one float32 multiply; -128 is -128 * step.
dequantize_f16  float32(x) of a float16 x: exact, infinities and NaN pass, subnormals are kept.
"""
import numpy as np

DEFAULT_STEP = np.float32(30 / 127)


def inv_step_of(step):
    return np.float32(1) / np.float32(step)


def _product(x, step):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(x).astype(np.float32) * inv_step_of(step)


def quantize(x, step=DEFAULT_STEP):
    p = _product(x, step)
    assert p.dtype == np.float32
    r = np.clip(np.rint(p), np.float32(-127), np.float32(127))
    return np.where(np.isnan(p), np.float32(0), r).astype(np.int8)


def saturated(x, step=DEFAULT_STEP):
    return int((np.abs(_product(x, step)) > np.float32(127)).sum())


def dequantize_i8(q, step=DEFAULT_STEP):
    q = np.asarray(q)
    assert q.dtype == np.int8
    out = q.astype(np.float32) * np.float32(step)
    assert out.dtype == np.float32
    return out


def dequantize_f16(x):
    x = np.asarray(x)
    assert x.dtype == np.float16
    return x.astype(np.float32)
