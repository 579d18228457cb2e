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


def equalize_device(syms, h, noise_var, coh=1, out=None, nv_out=None, stream=None):
    """Flat-fading equaliser: received complex64 [B, S] device
    symbols y = h x + n with known gains h, complex64 [B, ceil(S / coh)] (symbol s uses
    h[:, s // coh]), and the noise variance of y (a scalar, or a float64 [B] device
    tensor) -> (z = y / h complex64 [B, S], nv_sym = noise_var / |h|^2 float64 [B, S]),
    stream-ordered, for compute_llr_device / demap_planes_device to read in place.
    |h|^2 zero or not finite marks an erasure: z = 0, nv_sym = +inf (zero LLRs)."""
    import torch
    if not isinstance(syms, torch.Tensor) or syms.dtype != torch.complex64:
        raise TypeError(f"syms must be a torch.complex64 tensor, got {getattr(syms, 'dtype', type(syms))}")
    if not isinstance(h, torch.Tensor) or h.dtype != torch.complex64:
        raise TypeError(f"h must be a torch.complex64 tensor, got {getattr(h, 'dtype', type(h))}")
    if syms.dim() != 2 or syms.device.type != "cuda" or not syms.is_contiguous():
        raise ValueError("syms must be a contiguous 2-D [B, S] tensor on a HIP device")
    B, S = syms.shape
    coh = int(coh)
    if coh < 1:
        raise ValueError("coh must be >= 1")
    nh = -(-S // coh)
    if tuple(h.shape) != (B, nh) or not h.is_contiguous() or h.device != syms.device:
        raise ValueError(f"h must be a contiguous tensor of shape ({B}, {nh}) on the symbols' device, "
                         f"got {tuple(h.shape)}")
    rows = isinstance(noise_var, torch.Tensor)
    if rows:
        _nv_check(syms, noise_var, "row")
    if out is None:
        out = torch.empty_like(syms)
    elif out.dtype != torch.complex64 or tuple(out.shape) != (B, S) or not out.is_contiguous() or out.device != syms.device:
        raise ValueError(f"out must be a contiguous complex64 tensor of shape ({B}, {S}) on the symbols' device")
    if nv_out is None:
        nv_out = torch.empty((B, S), dtype=torch.float64, device=syms.device)
    else:
        _nv_check(syms, nv_out, "symbol", "nv_out")
    dev = syms.device.index or 0
    st = _n.stream_ptr(stream) if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    _n.check(_n.lib().tdec_equalize_dev(dev, _n.ptr(syms), _n.ptr(h), B, S, coh, 0.0 if rows else float(noise_var),
                                        _n.ptr(noise_var) if rows else None, _n.ptr(out), _n.ptr(nv_out), st))
    return out, nv_out


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
    st = _n.stream_ptr(stream) if stream is not None else torch.cuda.current_stream(dev).cuda_stream
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
    st = _n.stream_ptr(stream) if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    # tdec_demap[_rows][_logmap]_dev, or tdec_symnv_demap[_logmap]_dev for a per-symbol tensor:
    # (B, S) and the tensor for rows / syms, else n_sym and the scalar; no div_f32 for log-MAP
    stem = "tdec_symnv_demap" if form == "syms" else f"tdec_demap{'_rows' if rows else ''}"
    call = getattr(_n.lib(), f"{stem}{'_logmap' if lm else ''}_dev")
    _n.check(call(dev, _n.ptr(syms), int(sym_f64), *(syms.shape if rows else (n_sym,)), _n.ptr(c), int(f64), len(c),
                  m['bps'], _n.ptr(nvt) if rows else nv, *(() if lm else (int(div_f32),)), int(sign), _n.ptr(out), st))
    return out
