"""Soft-LLR demapper on MI355X: compute_llr of the reference harness
(test_sdr_with_coding.py:200-225) over the Gray constellations of the
reference (test_sdr_with_coding.py:25-100 for BPSK/QPSK/8PSK/16QAM,
sdr_modem.py:101-207 for 64QAM/256QAM).

``compute_llr(syms, mod_type, noise_var)`` returns exactly what the reference
returns (f64, positive for bit 1, clipped to +-30), including numpy's dtype
rules: the arithmetic is complex128 when the symbols or the constellation are
(QPSK's constellation is, because qpsk_mod divides by np.sqrt(2)), and the
final division stays float32 when noise_var ends up a Python float.
``sign=-1`` gives the decoder convention (positive for bit 0).

``algo="log-map"`` selects the exact log-sum demapper (build-defined, DESIGN.md
section 9), of which the reference's is the max-log approximation: the same
noise-variance floor, clip, sign and dtype rule, defined by a tolerance instead
of numpy's operation order.
"""
from __future__ import annotations

import numpy as np

from . import _native as _n

GRAY2 = [0, 1, 3, 2]
GRAY3 = [0, 1, 3, 2, 6, 7, 5, 4]
GRAY4 = [0, 1, 3, 2, 6, 7, 5, 4, 12, 13, 15, 14, 10, 11, 9, 8]


# ---- mappers: same expressions (and so the same rounding) as the reference -------------
def bpsk_mod(bits):                                   # test_sdr_with_coding.py:25-26
    return 2.0 * np.array(bits, dtype=np.complex64) - 1.0


def qpsk_mod(bits):                                   # :31-37
    bits = np.array(bits)
    if len(bits) % 2:
        bits = np.append(bits, 0)
    I = 1 - 2 * bits[0::2]
    Q = 1 - 2 * bits[1::2]
    return (I + 1j * Q).astype(np.complex64) / np.sqrt(2)


def psk8_mod(bits):                                   # :45-57 (sdr_modem.py:120-130)
    bits = np.array(bits)
    pad = (3 - len(bits) % 3) % 3
    if pad:
        bits = np.append(bits, [0] * pad)
    b = bits.reshape(-1, 3)
    idx = b[:, 0] * 4 + b[:, 1] * 2 + b[:, 2]
    phase = np.array(GRAY3)[idx] * np.pi / 4
    return np.array([np.exp(1j * p) for p in phase], dtype=np.complex64)


def _qam_mod(bits, k, gray, scale):
    bits = np.array(bits)
    pad = (2 * k - len(bits) % (2 * k)) % (2 * k)
    if pad:
        bits = np.append(bits, [0] * pad)
    b = bits.reshape(-1, 2 * k)
    w = 1 << np.arange(k - 1, -1, -1)
    i_idx = b[:, :k] @ w
    q_idx = b[:, k:] @ w
    M = 1 << k
    syms = [((2 * gray[i] - (M - 1)) / np.sqrt(scale)) + 1j * ((2 * gray[q] - (M - 1)) / np.sqrt(scale))
            for i, q in zip(i_idx, q_idx)]
    return np.array(syms, dtype=np.complex64)


def qam16_mod(bits):                                  # :72-86 (sdr_modem.py:142-154)
    return _qam_mod(bits, 2, GRAY2, 10)


def qam64_mod(bits):                                  # sdr_modem.py:168-180
    return _qam_mod(bits, 3, GRAY3, 42)


def qam256_mod(bits):                                 # sdr_modem.py:195-207
    return _qam_mod(bits, 4, GRAY4, 170)


MODULATIONS = {
    'BPSK': {'mod': bpsk_mod, 'bps': 1, 'order': 2},
    'QPSK': {'mod': qpsk_mod, 'bps': 2, 'order': 4},
    '8PSK': {'mod': psk8_mod, 'bps': 3, 'order': 8},
    '16QAM': {'mod': qam16_mod, 'bps': 4, 'order': 16},
    '64QAM': {'mod': qam64_mod, 'bps': 6, 'order': 64},
    '256QAM': {'mod': qam256_mod, 'bps': 8, 'order': 256},
}


def constellation(mod_type):
    """Label-ordered constellation, exactly as compute_llr builds it (:207-208)."""
    m = MODULATIONS[mod_type]
    bps, order = m['bps'], m['order']
    all_bits = np.array([list(map(int, format(i, f'0{bps}b'))) for i in range(order)])
    return m['mod'](all_bits.flatten()).reshape(-1)


_CONS = {}


def _cons(mod_type):
    c = _CONS.get(mod_type)
    if c is None:
        c = _CONS[mod_type] = constellation(mod_type)
    return c


def demap_mode(syms_dtype, cons_dtype, noise_var):
    """(f64 arithmetic?, float32 division?, effective noise_var) by numpy's rules."""
    nv = max(noise_var, 0.005)                                     # :202
    f64 = np.result_type(syms_dtype, cons_dtype) == np.complex128
    div_f32 = (not f64) and (np.float32(1) / nv).dtype == np.float32
    return f64, div_f32, float(nv)


ALGOS = ("max-log", "log-map")


def check_algo(algo):
    if algo not in ALGOS:
        raise ValueError(f"demapper algo must be one of {ALGOS}, not {algo!r}")
    return algo == "log-map"


def compute_llr(syms, mod_type, noise_var, sign=+1, device=0, algo="max-log"):
    """Soft demapper on the GPU: max-log (reference test_sdr_with_coding.py:200-225)
    or, with algo="log-map", the exact log-sum it approximates."""
    lm = check_algo(algo)
    m = MODULATIONS[mod_type]
    cons = _cons(mod_type)
    syms = np.asarray(syms)
    if syms.dtype not in (np.complex64, np.complex128):
        syms = syms.astype(np.complex128)
    syms = np.ascontiguousarray(syms)
    f64, div_f32, nv = demap_mode(syms.dtype, cons.dtype, noise_var)
    c = np.ascontiguousarray(cons.astype(np.complex128 if f64 else np.complex64))
    out = np.zeros(len(syms) * m['bps'])
    if len(syms) and lm:
        _n.check(_n.lib().tdec_demap_logmap(device, _n.ptr(syms), int(syms.dtype == np.complex128), len(syms),
                                            _n.ptr(c), int(f64), len(c), m['bps'], nv, int(sign), _n.ptr(out)))
    elif len(syms):
        _n.check(_n.lib().tdec_demap(device, _n.ptr(syms), int(syms.dtype == np.complex128), len(syms),
                                     _n.ptr(c), int(f64), len(c), m['bps'], nv, int(div_f32), int(sign),
                                     _n.ptr(out)))
    return out


def _nv_check(syms, nv, per, name="noise_var"):
    """A per-row (per = "row") or per-symbol ("symbol") noise
    variance: a contiguous float64 [B] or [B, S] tensor on the device of the 2-D [B, S]
    complex symbols.  Refused here, before any device call."""
    import torch
    if not isinstance(syms, torch.Tensor) or syms.dim() != 2 or not syms.is_complex():
        raise ValueError(f"a per-{per} {name} needs 2-D [B, S] complex symbols")
    if nv.dtype != torch.float64:
        raise TypeError(f"{name} must be torch.float64, got {nv.dtype}")
    want = tuple(syms.shape) if per == "symbol" else (syms.shape[0],)
    if tuple(nv.shape) != want or not nv.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor of shape {want}, got {tuple(nv.shape)}")
    if nv.device.type != "cuda" or nv.device != syms.device:
        raise ValueError(f"{name} must be on the symbols' HIP device")


def nv_tensor_form(syms, nv):
    """Which per-launch form a noise_var tensor is: "rows" ([B]) or "syms" ([B, S]), checked
    against the symbols."""
    if nv.dim() == 2:
        _nv_check(syms, nv, "symbol")
        return "syms"
    _nv_check(syms, nv, "row")
    return "rows"


def _stream_of(dev, stream):
    """The native handle of `stream`, or of the current stream of device index `dev`."""
    import torch
    return _n.stream_ptr(stream) if stream is not None else torch.cuda.current_stream(dev).cuda_stream


def _out_tensor(t, like, shape, dtype, name):
    """An output argument: a new tensor on the device of the input `like`, or the caller's, which must fit."""
    import torch
    if t is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
            or t.device != like.device):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the input's device")
    return t


MAX_BRANCHES = 8


def _syms_and_gains(syms, name, h, coh):
    """What equalize_device ([B, S] `syms`) and combine_device ([B, R, S] `y`) ask of their inputs:
    complex64 contiguous tensors on one HIP device, h with ceil(S / coh) gains per row.  -> int(coh)."""
    import torch
    for t, n in ((syms, name), (h, "h")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.complex64:
            raise TypeError(f"{n} must be a torch.complex64 tensor, got {getattr(t, 'dtype', type(t))}")
    ndim, dims = (2, "2-D [B, S]") if name == "syms" else (3, "3-D [B, R, S]")
    if syms.dim() != ndim or syms.device.type != "cuda" or not syms.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dims} tensor on a HIP device")
    if syms.dim() == 3 and not 1 <= syms.shape[1] <= MAX_BRANCHES:
        raise ValueError(f"1 .. {MAX_BRANCHES} branches, got {syms.shape[1]}")
    coh = int(coh)
    if coh < 1:
        raise ValueError("coh must be >= 1")
    want = (*syms.shape[:-1], -(-syms.shape[-1] // coh))
    if tuple(h.shape) != want or not h.is_contiguous() or h.device != syms.device:
        raise ValueError(f"h must be a contiguous tensor of shape {want} on the symbols' device, got {tuple(h.shape)}")
    return coh


def equalize_device(syms, h, noise_var, coh=1, out=None, nv_out=None, stream=None):
    """Flat-fading equaliser: received complex64 [B, S] device
    symbols y = h x + n with known gains h, complex64 [B, ceil(S / coh)] (symbol s uses
    h[:, s // coh]), and the noise variance of y (a scalar, or a float64 [B] device
    tensor) -> (z = y / h complex64 [B, S], nv_sym = noise_var / |h|^2 float64 [B, S]),
    stream-ordered, for compute_llr_device / demap_planes_device to read in place.
    |h|^2 zero or not finite marks an erasure: z = 0, nv_sym = +inf (zero LLRs)."""
    import torch
    coh = _syms_and_gains(syms, "syms", h, coh)
    B, S = syms.shape
    rows = isinstance(noise_var, torch.Tensor)
    if rows:
        _nv_check(syms, noise_var, "row")
    out = _out_tensor(out, syms, (B, S), torch.complex64, "out")
    nv_out = _out_tensor(nv_out, syms, (B, S), torch.float64, "nv_out")
    dev = syms.device.index or 0
    _n.check(_n.lib().tdec_equalize_dev(dev, _n.ptr(syms), _n.ptr(h), B, S, coh, 0.0 if rows else float(noise_var),
                                        _n.ptr(noise_var) if rows else None, _n.ptr(out), _n.ptr(nv_out),
                                        _stream_of(dev, stream)))
    return out, nv_out


def combine_device(y, h, noise_var, coh=1, out=None, nv_out=None, stream=None):
    """Maximal-ratio combiner of R receive branches: complex64
    [B, R, S] device symbols, branch r of burst b received through the known gains
    h[b, r], complex64 [B, R, ceil(S / coh)], -> (z complex64 [B, S], nv_sym float64 [B, S]),
    what equalize_device gives for one branch, stream-ordered, for compute_llr_device /
    demap_planes_device to read in place.  noise_var: a scalar or a float64 [B] device
    tensor (common to a burst's branches: z = sum conj(h) y / sum |h|^2, nv_sym = noise_var /
    sum |h|^2), or a float64 [B, R] device tensor (each branch its own: every term weighted
    by 1 / noise_var[b, r], nv_sym = 1 / sum (|h|^2 / noise_var)).  A branch whose |h|^2 is
    zero or not finite is skipped; with none left the symbol is an erasure, z = 0 and
    nv_sym = +inf (zero LLRs).  R = 1 with a common noise_var is equalize_device bit for bit."""
    import torch
    coh = _syms_and_gains(y, "y", h, coh)
    B, R, S = y.shape
    rows = branches = None
    if isinstance(noise_var, torch.Tensor):
        if noise_var.dtype != torch.float64:
            raise TypeError(f"noise_var must be torch.float64, got {noise_var.dtype}")
        if tuple(noise_var.shape) not in ((B,), (B, R)) or not noise_var.is_contiguous():
            raise ValueError(f"noise_var must be a contiguous tensor of shape ({B},) or ({B}, {R}), "
                             f"got {tuple(noise_var.shape)}")
        if noise_var.device != y.device:
            raise ValueError("noise_var must be on the symbols' HIP device")
        if noise_var.dim() == 2:
            branches = noise_var
        else:
            rows = noise_var
    out = _out_tensor(out, y, (B, S), torch.complex64, "out")
    nv_out = _out_tensor(nv_out, y, (B, S), torch.float64, "nv_out")
    dev = y.device.index or 0
    _n.check(_n.lib().tdec_combine_dev(dev, _n.ptr(y), _n.ptr(h), B, R, S, coh,
                                       0.0 if isinstance(noise_var, torch.Tensor) else float(noise_var),
                                       _n.ptr(rows), _n.ptr(branches), _n.ptr(out), _n.ptr(nv_out),
                                       _stream_of(dev, stream)))
    return out, nv_out


def stbc_coh(coh):
    """An Alamouti link's gain-block length in slots: an even int >= 2 (a pair never straddles two blocks)."""
    coh = int(coh)
    if coh < 2 or coh % 2:
        raise ValueError(f"transmit diversity needs an even coh >= 2 (a pair of slots shares its gains), got {coh}")
    return coh


def stbc_combine_device(y, h, noise_var, S=None, coh=2, out=None, nv_out=None, stream=None):
    """Alamouti 2 x R combiner (include/stbc.h): complex64 [B, R, S2]
    device slots, S2 even, branch r of burst b received from the two transmit antennas through
    the known effective gains h[b, r, 0] and h[b, r, 1], complex64 [B, R, 2, ceil(S2 / coh)]
    (E|h|^2 = 1/2 each at fixed total transmit power), -> (z complex64 [B, S], nv_sym float64
    [B, S]), what equalize_device and combine_device give, stream-ordered.  S: the codeword's
    symbols, S2 or (an odd S, passed explicitly) S2 - 1: the pad slot's second output is then not
    written.  noise_var: a scalar, a float64 [B] or a float64 [B, R] device tensor, as
    combine_device takes it.  A branch whose |h0|^2 + |h1|^2 is zero or not finite is skipped;
    with none left the pair is an erasure, z = 0 and nv_sym = +inf."""
    import torch
    for t, n in ((y, "y"), (h, "h")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.complex64:
            raise TypeError(f"{n} must be a torch.complex64 tensor, got {getattr(t, 'dtype', type(t))}")
    if y.dim() != 3 or y.shape[2] % 2:
        raise ValueError("y must be a 3-D [B, R, S2] tensor with an even S2 (pairs of slots)")
    if y.device.type != "cuda" or not y.is_contiguous():
        raise ValueError("y must be a contiguous 3-D [B, R, S2] tensor on a HIP device")
    B, R, S2 = y.shape
    if not 1 <= R <= MAX_BRANCHES:
        raise ValueError(f"1 .. {MAX_BRANCHES} branches, got {R}")
    coh = stbc_coh(coh)
    S = S2 if S is None else int(S)
    if S < 0 or S not in (S2, S2 - 1):
        raise ValueError(f"S must be S2 = {S2} or the odd S2 - 1, got {S}")
    want = (B, R, 2, -(-S2 // coh))
    if h.dim() != 4 or tuple(h.shape) != want or not h.is_contiguous() or h.device != y.device:
        raise ValueError(f"h must be a contiguous 4-D tensor of shape {want} on the symbols' device, "
                         f"got {tuple(h.shape)}")
    rows = branches = None
    if isinstance(noise_var, torch.Tensor):
        if noise_var.dtype != torch.float64:
            raise TypeError(f"noise_var must be torch.float64, got {noise_var.dtype}")
        if tuple(noise_var.shape) not in ((B,), (B, R)) or not noise_var.is_contiguous():
            raise ValueError(f"noise_var must be a contiguous tensor of shape ({B},) or ({B}, {R}), "
                             f"got {tuple(noise_var.shape)}")
        if noise_var.device != y.device:
            raise ValueError("noise_var must be on the symbols' HIP device")
        if noise_var.dim() == 2:
            branches = noise_var
        else:
            rows = noise_var
    out = _out_tensor(out, y, (B, S), torch.complex64, "out")
    nv_out = _out_tensor(nv_out, y, (B, S), torch.float64, "nv_out")
    dev = y.device.index or 0
    _n.check(_n.lib().stbc_combine_dev(dev, _n.ptr(y), _n.ptr(h), B, R, S, coh,
                                       0.0 if isinstance(noise_var, torch.Tensor) else float(noise_var),
                                       _n.ptr(rows), _n.ptr(branches), _n.ptr(out), _n.ptr(nv_out),
                                       _stream_of(dev, stream)))
    return out, nv_out


SM_MAX_ORDER = 64                                     # the joint detector searches M^2 hypotheses per slot


def sm_order(mod_type):
    """(constellation, bps) of a modulation the joint detector takes: up to 64 points."""
    m = MODULATIONS[mod_type]
    if m['order'] > SM_MAX_ORDER:
        raise ValueError(f"spatial multiplexing detects up to {SM_MAX_ORDER}-point constellations jointly, "
                         f"not {mod_type}")
    return _cons(mod_type), m['bps']


def sm_detect_device(y, h, mod_type, noise_var, S=None, coh=1, out=None, sign=+1, stream=None):
    """2 x R joint max-log detector of a spatially multiplexed link (DESIGN.md section 19,
    include/sm.h): complex64 [B, R, T] device slots, slot m carrying x[2m] from antenna 0 and
    x[2m+1] from antenna 1 through the known effective gains h[b, r, 0] and h[b, r, 1], complex64
    [B, R, 2, ceil(T / coh)] -> float32 [B, S * bps] LLRs, symbol s, bit j at s * bps + j, clipped
    to +-30, stream-ordered.  S: the codeword's symbols, 2 T or (an odd S, passed explicitly)
    2 T - 1: antenna 1 is then silent in the last slot.  noise_var: a scalar, a float64 [B] or a
    float64 [B, R] device tensor, floored at 0.005 on the device.  sign as compute_llr's (-1: the
    decoder's).  out: a float32 [B, S * bps] tensor, or a [B, >= S * bps] view of rows whose
    elements are contiguous (a column slice of a wider buffer: its row stride is passed on).
    max-log only; 256QAM is refused."""
    import torch
    cons, bps = sm_order(mod_type)
    for t, n in ((y, "y"), (h, "h")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.complex64:
            raise TypeError(f"{n} must be a torch.complex64 tensor, got {getattr(t, 'dtype', type(t))}")
    if y.dim() != 3:
        raise ValueError("y must be a 3-D [B, R, T] tensor (one slot per pair of symbols)")
    if y.device.type != "cuda" or not y.is_contiguous():
        raise ValueError("y must be a contiguous 3-D [B, R, T] tensor on a HIP device")
    B, R, T = y.shape
    if not 1 <= R <= MAX_BRANCHES:
        raise ValueError(f"1 .. {MAX_BRANCHES} branches, got {R}")
    coh = int(coh)
    if coh < 1:
        raise ValueError("coh must be >= 1")
    S = 2 * T if S is None else int(S)
    if S < 0 or S not in (2 * T, 2 * T - 1):
        raise ValueError(f"S must be 2 T = {2 * T} or the odd 2 T - 1, got {S}")
    want = (B, R, 2, -(-T // coh))
    if h.dim() != 4 or tuple(h.shape) != want or not h.is_contiguous() or h.device != y.device:
        raise ValueError(f"h must be a contiguous 4-D tensor of shape {want} on the symbols' device, "
                         f"got {tuple(h.shape)}")
    rows = branches = None
    if isinstance(noise_var, torch.Tensor):
        if noise_var.dtype != torch.float64:
            raise TypeError(f"noise_var must be torch.float64, got {noise_var.dtype}")
        if tuple(noise_var.shape) not in ((B,), (B, R)) or not noise_var.is_contiguous():
            raise ValueError(f"noise_var must be a contiguous tensor of shape ({B},) or ({B}, {R}), "
                             f"got {tuple(noise_var.shape)}")
        if noise_var.device != y.device:
            raise ValueError("noise_var must be on the symbols' HIP device")
        if noise_var.dim() == 2:
            branches = noise_var
        else:
            rows = noise_var
    if sign not in (1, -1):
        raise ValueError(f"sign must be +1 or -1, got {sign!r}")
    L = S * bps
    if out is None:
        out = torch.empty((B, L), dtype=torch.float32, device=y.device)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (B, L)
            or out.device != y.device or (L > 1 and out.stride(1) != 1) or (B > 1 and out.stride(0) < L)):
        raise ValueError(f"out must be a float32 tensor of shape ({B}, {L}) on the input's device whose rows are "
                         "contiguous")
    stride = out.stride(0) if B > 1 else L
    c = np.ascontiguousarray(cons)
    dev = y.device.index or 0
    _n.check(_n.lib().sm_detect_dev(dev, _n.ptr(y), _n.ptr(h), B, R, S, coh, _n.ptr(c), int(c.dtype == np.complex128),
                                    len(c), 0.0 if isinstance(noise_var, torch.Tensor) else float(noise_var),
                                    _n.ptr(rows), _n.ptr(branches), int(sign), _n.ptr(out), int(stride),
                                    _stream_of(dev, stream)))
    return out


def estimate_noise_var_device(syms, mod_type, floor=0.02, out=None, stream=None):
    """The receiver's decision-directed noise variance (test_sdr_with_coding.py:459-467:
    hard decision, re-map, mean |rx - const|^2, max(nv, 0.02)) of each row of complex64
    [B, S] device symbols: a float64 [B] tensor on their device, stream-ordered, for
    compute_llr_device / demap_planes_device / DevicePipeline.run to read in place.
    Build-defined: the f64 mean of the f64 squared distances."""
    import torch
    cons = _cons(mod_type)
    if not isinstance(syms, torch.Tensor) or syms.dtype != torch.complex64:
        raise TypeError(f"syms must be a torch.complex64 tensor, got {getattr(syms, 'dtype', type(syms))}")
    if syms.dim() != 2 or syms.shape[1] < 1:
        raise ValueError("syms must be 2-D [B, S] with S >= 1")
    if syms.device.type != "cuda" or not syms.is_contiguous():
        raise ValueError("syms must be a contiguous tensor on a HIP device")
    B, S = syms.shape
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=syms.device)
    else:
        _nv_check(syms, out, "row", "out")
    f64 = cons.dtype == np.complex128
    c = np.ascontiguousarray(cons.astype(np.complex128 if f64 else np.complex64))
    dev = syms.device.index or 0
    st = _stream_of(dev, stream)
    _n.check(_n.lib().tdec_noise_var_dev(dev, _n.ptr(syms), B, S, _n.ptr(c), int(f64), len(c), float(floor),
                                         _n.ptr(out), st))
    return out


def compute_llr_device(syms, mod_type, noise_var, out=None, sign=+1, stream=None, algo="max-log"):
    """compute_llr over a device tensor of complex symbols (complex64/complex128 or
    a float [..., 2] view); returns a float64 device tensor.  noise_var: a scalar, or
    a float64 [B] device tensor with 2-D [B, S] symbols (row r demapped with
    noise_var[r], read on the device: no host round trip), or a float64 [B, S] one
    (symbol (r, s) with noise_var[r, s], equalize_device's nv_sym);
    the result is then [B, S*bps]."""
    import torch
    lm = check_algo(algo)
    m = MODULATIONS[mod_type]
    cons = _cons(mod_type)
    rows = isinstance(noise_var, torch.Tensor)
    form = nv_tensor_form(syms, noise_var) if rows else ""
    sym_f64 = syms.dtype in (torch.complex128, torch.float64)
    n_sym = syms.numel() // (1 if syms.is_complex() else 2)
    if rows:   # the division's dtype: what a numpy float64 scalar gives (as DevicePipeline.run treats its scalar)
        noise_var, nvt = np.float64(1.0), noise_var
    f64, div_f32, nv = demap_mode(np.complex128 if sym_f64 else np.complex64, cons.dtype, noise_var)
    c = np.ascontiguousarray(cons.astype(np.complex128 if f64 else np.complex64))
    if syms.device.type != "cuda" or not syms.is_contiguous():
        raise ValueError("syms must be a contiguous tensor on a HIP device")
    if syms.dtype not in (torch.complex64, torch.complex128, torch.float32, torch.float64):
        raise TypeError(f"unsupported symbol dtype {syms.dtype}")
    dev = syms.device.index or 0
    if out is None:
        out = torch.empty((syms.shape[0], syms.shape[1] * m['bps']) if rows else n_sym * m['bps'],
                          dtype=torch.float64, device=syms.device)
    if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() < n_sym * m['bps'] or out.device != syms.device:
        raise ValueError("out must be a contiguous float64 tensor of n_sym*bps elements on the symbols' device")
    st = _stream_of(dev, stream)
    # tdec_demap[_rows][_logmap]_dev, or tdec_symnv_demap[_logmap]_dev for a per-symbol tensor:
    # (B, S) and the tensor for rows / syms, else n_sym and the scalar; no div_f32 for log-MAP
    stem = "tdec_symnv_demap" if form == "syms" else f"tdec_demap{'_rows' if rows else ''}"
    call = getattr(_n.lib(), f"{stem}{'_logmap' if lm else ''}_dev")
    _n.check(call(dev, _n.ptr(syms), int(sym_f64), *(syms.shape if rows else (n_sym,)), _n.ptr(c), int(f64), len(c),
                  m['bps'], _n.ptr(nvt) if rows else nv, *(() if lm else (int(div_f32),)), int(sign), _n.ptr(out), st))
    return out


# ---- quantised LLRs ----------------------------------------------
LLR_DEFAULT_STEP = _n.LLRQ_DEFAULT_STEP               # float32(30 / 127): compute_llr clips to +-30


def quantize_llr_device(llr, step=LLR_DEFAULT_STEP, out=None, count_saturated=False, stream=None):
    """int8 soft bits of a float32 or float64 device tensor of LLRs (llrq_quantize_dev,
    include/llrq.h): q = clamp(rint(float32(x) * inv_step), -127, 127), ties to even, with
    inv_step = float32(1) / float32(step) formed here; NaN -> 0, +-inf -> +-127.  Any shape and
    any view whose elements are contiguous (a sliced base needs no alignment); the result has
    the input's shape.  The decoder widens q as float32(q) * step (decode_device(llr_step=step)).
    count_saturated: an int64 [1] device tensor to ADD the number of elements with
    |x * inv_step| > 127 to, or True for a fresh one; the result is then (q, counter)."""
    import torch
    if not isinstance(llr, torch.Tensor) or llr.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"llr must be a float32 or float64 tensor, got {getattr(llr, 'dtype', type(llr))}")
    if llr.device.type != "cuda" or not llr.is_contiguous():
        raise ValueError("llr must be a contiguous tensor on a HIP device")
    step = np.float32(step)
    if not np.isfinite(step) or step <= 0:
        raise ValueError("step must be finite and > 0")
    inv_step = np.float32(1) / step
    if not np.isfinite(inv_step):
        raise ValueError("1 / step must be finite in float32")
    out = _out_tensor(out, llr, llr.shape, torch.int8, "out")
    sat = None
    if count_saturated is True:
        sat = torch.zeros(1, dtype=torch.int64, device=llr.device)
    elif count_saturated is not False and count_saturated is not None:
        sat = count_saturated
        if (not isinstance(sat, torch.Tensor) or sat.dtype != torch.int64 or sat.numel() != 1
                or sat.device != llr.device):
            raise ValueError("count_saturated must be True or an int64 [1] tensor on the input's device")
    dev = llr.device.index or 0
    _n.check(_n.lib().llrq_quantize_dev(dev, _n.ptr(llr), int(llr.dtype == torch.float64), llr.numel(), inv_step,
                                        _n.ptr(out), _n.ptr(sat), _stream_of(dev, stream)))
    return (out, sat) if sat is not None else out


# ---- pilot-aided channel estimation ------------------------------
CSI_MODES = {"linear": 0, "mean": 1}
CSI_MAX_BLOCKS = 2048                                 # pilot blocks per burst the estimator's LDS holds


class PilotLayout:
    """A framed burst: J + 1 pilot blocks of `plen` symbols around J = ceil(S / dlen) data
    segments of `dlen` symbols (the last may be short), P0 D0 P1 D1 ... D(J-1) PJ.

    The pilot sequence is shared by all rows.  By default pilot k of the frame (counted
    over the pilots alone) is 1j ** ((k * (k + 1) // 2) % 4): unit modulus, QPSK phases, an
    integer formula and no RNG.  `sequence`, a complex array, replaces it; a burst of S data
    symbols takes its first (J + 1) * plen values.  A pilot block of zero energy is refused."""

    def __init__(self, plen, dlen, sequence=None):
        plen, dlen = int(plen), int(dlen)
        if plen < 1 or dlen < 1:
            raise ValueError("PilotLayout needs plen >= 1 and dlen >= 1")
        self.plen, self.dlen = plen, dlen
        self.sequence = None if sequence is None else np.asarray(sequence).astype(np.complex64).reshape(-1)
        self._dev = {}

    def n_segments(self, S):
        """J = ceil(S / dlen)."""
        if int(S) < 1:
            raise ValueError("a burst needs S >= 1 data symbols")
        return -(-int(S) // self.dlen)

    def n_blocks(self, S):
        return self.n_segments(S) + 1

    def frame_len(self, S):
        """T = S + (J + 1) * plen."""
        return int(S) + self.n_blocks(S) * self.plen

    def segment_len(self, S, j):
        """L_j: data symbols [j * dlen, min((j + 1) * dlen, S))."""
        if not 0 <= j < self.n_segments(S):
            raise IndexError(f"segment {j} of {self.n_segments(S)}")
        return min(self.dlen, int(S) - j * self.dlen)

    def block_start(self, S, j):
        """Frame position of the first pilot of block j."""
        J = self.n_segments(S)
        if not 0 <= j <= J:
            raise IndexError(f"pilot block {j} of {J + 1}")
        return j * (self.plen + self.dlen) if j < J else int(S) + J * self.plen

    def data_positions(self, S):
        """Frame position of each data symbol, int64 [S]."""
        s = np.arange(int(S), dtype=np.int64)
        return s + (s // self.dlen + 1) * self.plen

    def pilot_positions(self, S):
        """Frame position of each pilot, int64 [(J + 1) * plen], block by block."""
        return np.concatenate([self.block_start(S, j) + np.arange(self.plen, dtype=np.int64)
                               for j in range(self.n_blocks(S))])

    def pilots(self, S):
        """The burst's pilot sequence, complex64 [(J + 1) * plen]."""
        n = self.n_blocks(S) * self.plen
        if self.sequence is None:
            k = np.arange(n, dtype=np.int64)
            q = (k * (k + 1) // 2) % 4
            p = np.empty(n, np.complex64)
            p.real = np.array([1, 0, -1, 0], np.float32)[q]
            p.imag = np.array([0, 1, 0, -1], np.float32)[q]
        else:
            if len(self.sequence) < n:
                raise ValueError(f"the pilot sequence has {len(self.sequence)} values; S = {S} needs {n}")
            p = self.sequence[:n]
        e = (np.abs(p.astype(np.complex128)) ** 2).reshape(-1, self.plen).sum(axis=1)
        if not np.all(e > 0):                         # (also refuses a NaN block)
            raise ValueError(f"pilot block {int(np.flatnonzero(~(e > 0))[0])} has no energy")
        return np.ascontiguousarray(p)

    def pilots_device(self, S, device):
        """pilots(S) on `device`, uploaded once per (S, device)."""
        import torch
        key = (int(S), str(device))
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = torch.from_numpy(self.pilots(S)).to(device)
        return t


def _csi_frames_check(frames, layout, mode, need_residual=False):
    """(B, S) of a framed batch.  Every refusal comes before any device call, and in an order
    that lets each be met with host tensors: layout, mode and noise source, dtype, shape, the
    pilot blocks' energy, then device and contiguity."""
    import torch
    if not isinstance(layout, PilotLayout):
        raise TypeError(f"layout must be a PilotLayout, got {type(layout)}")
    if mode not in CSI_MODES:
        raise ValueError(f"mode must be one of {tuple(CSI_MODES)}, not {mode!r}")
    if need_residual and layout.plen < 2:
        raise ValueError("plen == 1 leaves no residual to estimate the noise from: pass noise_var "
                         "(and no nv_rows_out)")
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.complex64:
        raise TypeError(f"frames must be a torch.complex64 tensor, got {getattr(frames, 'dtype', type(frames))}")
    if frames.dim() != 2:
        raise ValueError("frames must be a 2-D [B, T] tensor")
    B, T = frames.shape
    # T = S + (ceil(S / dlen) + 1) * plen is increasing in S: the one S that gives T, if any
    full, rest = divmod(T - layout.plen, layout.plen + layout.dlen)
    S = full * layout.dlen + (rest - layout.plen if rest else 0)
    if B < 1 or S < 1 or (rest and rest <= layout.plen) or layout.frame_len(S) != T:
        raise ValueError(f"frames must be [B >= 1, T] with T the frame length of some S >= 1 for plen = "
                         f"{layout.plen}, dlen = {layout.dlen}; got {tuple(frames.shape)}")
    if layout.n_blocks(S) > CSI_MAX_BLOCKS:
        raise ValueError(f"more than {CSI_MAX_BLOCKS} pilot blocks per burst")
    layout.pilots(S)                                  # refuses a zero-energy block
    return B, S


def _csi_device_check(frames):
    if frames.device.type != "cuda" or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous tensor on a HIP device")


def estimate_csi_device(frames, layout, noise_var=None, mode="linear", floor=0.02, out=None, nv_out=None, h_out=None,
                        nv_rows_out=None, stream=None):
    """Pilot-aided channel estimation and equalisation in one launch:
    framed complex64 [B, T] device bursts (layout: PilotLayout) -> (z complex64 [B, S],
    nv_sym float64 [B, S]), what equalize_device gives for the stripped data, the gains
    interpolated between the pilot blocks' estimates (mode "linear", or "mean": the midpoint
    of the two bordering blocks for the whole segment) and the burst's noise variance.

    noise_var: a scalar, a float64 [B] device tensor, or None: estimated from the pilots'
    residuals, max(mean, floor) per row, which needs plen >= 2.  h_out (complex64 [B, S]) and
    nv_rows_out (float64 [B], plen >= 2) receive the gains and the estimate when given.
    A non-finite or all-zero received pilot block erases the segments it borders."""
    import torch
    B, S = _csi_frames_check(frames, layout, mode, need_residual=noise_var is None or nv_rows_out is not None)
    rows = isinstance(noise_var, torch.Tensor)
    if rows:
        if noise_var.dtype != torch.float64:
            raise TypeError(f"noise_var must be torch.float64, got {noise_var.dtype}")
        if tuple(noise_var.shape) != (B,) or not noise_var.is_contiguous():
            raise ValueError(f"noise_var must be a contiguous tensor of shape ({B},), got {tuple(noise_var.shape)}")
    elif noise_var is not None and float(noise_var) < 0:
        raise ValueError("noise_var must not be negative")
    _csi_device_check(frames)
    if rows and noise_var.device != frames.device:
        raise ValueError("noise_var must be on the frames' HIP device")
    pil = layout.pilots_device(S, frames.device)
    out = _out_tensor(out, frames, (B, S), torch.complex64, "out")
    nv_out = _out_tensor(nv_out, frames, (B, S), torch.float64, "nv_out")
    if h_out is not None:
        h_out = _out_tensor(h_out, frames, (B, S), torch.complex64, "h_out")
    if nv_rows_out is not None:
        nv_rows_out = _out_tensor(nv_rows_out, frames, (B,), torch.float64, "nv_rows_out")
    dev = frames.device.index or 0
    st = _stream_of(dev, stream)
    _n.check(_n.lib().tdec_csi_pilots_dev(dev, _n.ptr(frames), B, S, layout.plen, layout.dlen, _n.ptr(pil),
                                          CSI_MODES[mode], -1.0 if rows or noise_var is None else float(noise_var),
                                          _n.ptr(noise_var) if rows else None, float(floor), _n.ptr(out),
                                          _n.ptr(nv_out), _n.ptr(h_out), _n.ptr(nv_rows_out), st))
    return out, nv_out


def strip_pilots_device(frames, layout, mode="linear", floor=0.02, out=None, h_out=None, nv_rows_out=None, stream=None):
    """The unfused form of estimate_csi_device: (y complex64 [B, S], the stripped data, and
    h complex64 [B, S], the interpolated gains), for equalize_device(y, h, nv, coh=1) to
    follow; nv_rows_out (float64 [B], plen >= 2) receives the pilots' noise estimate."""
    import torch
    B, S = _csi_frames_check(frames, layout, mode, need_residual=nv_rows_out is not None)
    _csi_device_check(frames)
    pil = layout.pilots_device(S, frames.device)
    out = _out_tensor(out, frames, (B, S), torch.complex64, "out")
    h_out = _out_tensor(h_out, frames, (B, S), torch.complex64, "h_out")
    if nv_rows_out is not None:
        nv_rows_out = _out_tensor(nv_rows_out, frames, (B,), torch.float64, "nv_rows_out")
    dev = frames.device.index or 0
    st = _stream_of(dev, stream)
    _n.check(_n.lib().tdec_csi_strip_dev(dev, _n.ptr(frames), B, S, layout.plen, layout.dlen, _n.ptr(pil),
                                         CSI_MODES[mode], float(floor), _n.ptr(out), _n.ptr(h_out),
                                         _n.ptr(nv_rows_out), st))
    return out, h_out
