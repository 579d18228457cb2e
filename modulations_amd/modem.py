"""Modem front-end on MI355X: the reference's symbol
mappers, hard-decision demodulators, RRC pulse shaping / matched filtering
and int8/uint8 IQ sample format, behind the reference's own names.

  SDRModem            sdr_modem.py:17-385, 523-664 (mappers, demods,
                      _rrc_filter, _upsample_filter, modulate/demodulate,
                      _save_iq/_load_iq, build_frame and the burst-receive
                      chain: _estimate_freq_offset, _correct_freq, both carrier
                      loops, _process_received; the radio I/O of transmit /
                      receive / receive_and_transmit is out of scope)
  Modulator,          modulators.py:19-199 (natural-label mappers, argmin QAM
  rrcosfilter         demods, upfirdn pulse shaping, matched filter)
  bpsk_mod ...        test_sdr_with_coding.py:25-128, 228-240 (the harness
  rrc_taps, ...       copies: mappers/demods, rrc_taps, upsample_filter,
  save_iq, load_iq    save_iq, load_iq)

Host work is limited to setup the reference also does once per call or per
object -- constellation tables, label maps and filter taps, built with the
reference's own numpy expressions -- and file I/O.  Every per-symbol and
per-sample operation runs in libmodem.so (include/modem.h) on the GPU; there
is no CPU fallback.  Outputs keep the reference's dtypes (int64 bits,
complex64/complex128 symbols, complex128 filter outputs).

Deliberate deviations, all documented in DESIGN.md §3: bits must be 0/1 (the
reference's integer arithmetic on other values has no table form); the
int8 conversion of _save_iq takes complex input (a real array is treated as
complex with zero imaginary part, which numpy would divide without Smith's
method); SDRModem.sync_syms is computed on first use instead of in __init__.
"""
from __future__ import annotations

import numpy as np

from . import _native as _n
from . import demap as D

# ---------------------------------------------------------------- C-ABI wrappers ------------
GT0, QPSK, PSK8, QAM_AXIS, ARGMIN = 0, 1, 2, 3, 4


def _bits_u8(bits):
    b = np.asarray(bits)
    if b.dtype == np.uint8 and b.flags.c_contiguous:
        u = b.ravel()
    else:
        u = np.ascontiguousarray(b.ravel())
        if u.size and not np.all((u == 0) | (u == 1)):
            raise ValueError("bits must be 0 or 1")
        u = u.astype(np.uint8)
    if u.size and u.max(initial=0) > 1:
        raise ValueError("bits must be 0 or 1")
    return u


_p = _n.ptr


def _call(name, *args):
    """One call of the libmodem.so export `name`, its status through modem_check."""
    _n.modem_check(getattr(_n.modem_lib(), name)(*args))


def _ordinal(t):
    """The device ordinal of a tensor, as the _dev forms take it."""
    return t.device.index or 0


_F64 = {}


def _f64(a):
    """The library's sample-type flag of an array or a tensor: 1 for complex128, 0 for complex64."""
    f = _F64.get(a.dtype)
    if f is None:      # numpy's and torch's complex128, each dtype's name looked at once
        f = _F64[a.dtype] = int(str(a.dtype).endswith("complex128"))
    return f


def _out(t, like, shape, dtype):
    """An output argument of a device form: the caller's as it is, or a new tensor on the device of `like`."""
    if t is not None:
        return t
    import torch
    return torch.empty(shape, dtype=getattr(torch, dtype), device=like.device)


def map_bits(bits, bps, table, device=0):
    """Labels (MSB first, zero-padded to whole symbols) -> table[label] on the GPU."""
    table = np.ascontiguousarray(table)
    assert table.dtype in (np.complex64, np.complex128) and table.size == 1 << bps
    u = _bits_u8(bits)
    out = np.empty(-(-u.size // bps), table.dtype)
    if u.size:
        _call("mdm_map", device, _p(u), u.size, bps, _p(table), _f64(table), _p(out))
    return out


def _syms_c(syms):
    s = np.asarray(syms)
    if s.dtype not in (np.complex64, np.complex128):
        s = s.astype(np.complex128)
    return np.ascontiguousarray(s.ravel())


def _demod_tables(labels, cons):
    return (None if labels is None else np.ascontiguousarray(labels, np.int32),
            None if cons is None else np.ascontiguousarray(cons, np.complex128))


def hard_demod(syms, kind, bps, labels=None, scale=0.0, cons=None, nan_raises=True, device=0):
    """uint8 bits [n_sym * bps] of the given rule (include/modem.h MDM_DEMOD_*)."""
    s = _syms_c(syms)
    out = np.empty(s.size * bps, np.uint8)
    lab, c = _demod_tables(labels, cons)
    if s.size:
        _call("mdm_demod", device, kind, _p(s), _f64(s), s.size, bps, _p(lab), float(scale), _p(c),
              int(bool(nan_raises)), _p(out))
    return out


def fir(x, taps, up=1, down=1, offset=0, n_out=None, device=0):
    """out[i] = sum_k taps[k] * xu[i*down + offset - k] (complex128), see modem.h."""
    s = _syms_c(x)
    h = np.ascontiguousarray(taps, np.float64)
    out = np.empty(n_out, np.complex128)
    if n_out:
        _call("mdm_fir", device, _p(s), _f64(s), s.size, _p(h), h.size, up, down, offset, n_out, _p(out))
    return out


def iq_quantize(sig, device=0):
    """_save_iq's int8 interleaved samples of a complex signal."""
    s = _syms_c(sig)
    if s.size == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    out = np.empty(2 * s.size, np.int8)
    _call("mdm_iq_quantize", device, _p(s), _f64(s), s.size, _p(out))
    return out


def iq_dequantize(raw, device=0):
    """_load_iq's complex64 samples of interleaved uint8 I/Q bytes."""
    r = np.ascontiguousarray(np.asarray(raw, np.uint8).ravel())
    if r.size % 2:
        # raw[0::2] has one sample more than raw[1::2]: I + 1j * Q broadcasts
        # only when Q has 0 or 1 samples, as numpy does
        if r.size == 1:
            return np.zeros(0, np.complex64)
        if r.size == 3:
            r = np.array([r[0], r[1], r[2], r[1]], np.uint8)
        else:
            raise ValueError(f"operands could not be broadcast together with shapes ({r.size // 2 + 1},) "
                             f"({r.size // 2},)")
    out = np.empty(r.size // 2, np.complex64)
    if out.size:
        _call("mdm_iq_dequantize", device, _p(r), out.size, _p(out))
    return out


# ---- device-resident forms (torch tensors on the GPU, stream-ordered) ----------------------
def map_device(bits, bps, table, out=None, stream=None):
    table = np.ascontiguousarray(table)
    out = _out(out, bits, -(-bits.numel() // bps), "complex128" if _f64(table) else "complex64")
    _call("mdm_map_dev", _ordinal(bits), _p(bits), bits.numel(), bps, _p(table), _f64(table), _p(out),
          _n.stream_ptr(stream))
    return out


def demod_device(syms, kind, bps, labels=None, scale=0.0, cons=None, nan_raises=True, out=None, nan_count=None,
                 stream=None):
    lab, c = _demod_tables(labels, cons)
    out = _out(out, syms, syms.numel() * bps, "uint8")
    _call("mdm_demod_dev", _ordinal(syms), kind, _p(syms), _f64(syms), syms.numel(), bps, _p(lab), float(scale), _p(c),
          int(bool(nan_raises)), _p(out), _p(nan_count), _n.stream_ptr(stream))
    return out


def fir_device(x, taps, up=1, down=1, offset=0, n_out=None, out=None, stream=None):
    h = np.ascontiguousarray(taps, np.float64)
    out = _out(out, x, n_out, "complex128")
    _call("mdm_fir_dev", _ordinal(x), _p(x), _f64(x), x.numel(), _p(h), h.size, up, down, offset, n_out, _p(out),
          _n.stream_ptr(stream))
    return out


def iq_quantize_device(sig, out=None, scratch=None, stream=None):
    out = _out(out, sig, 2 * sig.numel(), "int8")
    scratch = _out(scratch, sig, 1, "int64")
    _call("mdm_iq_quantize_dev", _ordinal(sig), _p(sig), _f64(sig), sig.numel(), _p(out), _p(scratch),
          _n.stream_ptr(stream))
    return out


def iq_dequantize_device(raw, out=None, stream=None):
    n = raw.numel() // 2
    out = _out(out, raw, n, "complex64")
    _call("mdm_iq_dequantize_dev", _ordinal(raw), _p(raw), n, _p(out), _n.stream_ptr(stream))
    return out


# ---- burst-receive chain (include/modem.h: mixer, burst detector, sync search, carrier loops) ----
CR_BPSK, CR_QUAD, CR_PSK8 = 0, 1, 2
XCORR_MAX_TAPS = 1024      # sync waveform taps of mdm_xcorr_peak
BURST_MAX_WIN = 1024       # smoothing window of mdm_burst_find
_RX_TILE = 1024            # outputs per workgroup: the scratch buffers hold 16 bytes per tile


def _dc(dc):
    if dc is None:
        return None
    z = complex(dc)
    return np.array([z.real, z.imag], np.float64)


def _check_burst(n, win, preamble_len):
    if not 1 <= win <= BURST_MAX_WIN:
        raise ValueError(f"smoothing window must be 1..{BURST_MAX_WIN} samples")
    if n < win:
        raise ValueError("capture shorter than the smoothing window")
    if preamble_len < 0:
        raise ValueError("negative preamble length")


def _check_xcorr(n_region, n_w):
    if not 1 <= n_w <= XCORR_MAX_TAPS:
        raise ValueError(f"sync waveform must have 1..{XCORR_MAX_TAPS} taps")
    if n_region < n_w:
        raise ValueError("search region shorter than the sync waveform")


def _carrier_params(n_cand, init_phase, init_freq, alpha, kind):
    """Per-candidate parameter arrays; scalars apply to every candidate."""
    out = []
    for name, v, dt in (("init_phase", init_phase, np.float64), ("init_freq", init_freq, np.float64),
                        ("alpha", alpha, np.float64), ("kind", kind, np.int32)):
        a = np.asarray(v)
        if a.ndim == 0:
            a = np.full(n_cand, a)
        if a.shape != (n_cand,):
            raise ValueError(f"{name} has shape {a.shape}, expected ({n_cand},) for {n_cand} candidate streams")
        out.append(np.ascontiguousarray(a.astype(dt)))
    if out[3].size and not np.all((out[3] >= CR_BPSK) & (out[3] <= CR_PSK8)):
        raise ValueError("unknown carrier detector kind")
    return out


def mix(sig, w, fs, dc=None, i0=0, device=0):
    """(sig - dc) * exp(1j * w * (i0 + arange(n)) / fs), complex128 (mdm_mix, _correct_freq)."""
    s = _syms_c(sig)
    out = np.empty(s.size, np.complex128)
    dcv = _dc(dc)              # held here: the library reads it during the call
    if s.size:
        _call("mdm_mix", device, _p(s), _f64(s), s.size, int(i0), _p(dcv), float(w), float(fs), _p(out))
    return out


def burst_find(sig, preamble_len, win=1000, dc=None, want_smooth=False, device=0):
    """(burst_start or -1, max smoothed power, smoothed power or None) of mdm_burst_find.
    dc: np.mean(sig), formed by the caller on the host."""
    s = _syms_c(sig)
    _check_burst(s.size, win, preamble_len)
    start, mx = np.zeros(1, np.int64), np.zeros(1, np.float64)
    smooth = np.empty(s.size, np.float64) if want_smooth else None
    dcv = _dc(dc)
    _call("mdm_burst_find", device, _p(s), _f64(s), s.size, _p(dcv), int(win), int(preamble_len), _p(start), _p(mx),
          _p(smooth))
    return int(start[0]), float(mx[0]), smooth


def xcorr_peak(region, wave, want_corr=False, device=0):
    """(argmax, peak, corr or None) of |correlate(region, wave, 'valid')| (mdm_xcorr_peak)."""
    r = np.ascontiguousarray(np.asarray(region).ravel().astype(np.complex128, copy=False))
    h = np.ascontiguousarray(np.asarray(wave).ravel().astype(np.complex128, copy=False))
    _check_xcorr(r.size, h.size)
    idx, peak = np.zeros(1, np.int64), np.zeros(1, np.float64)
    corr = np.empty(r.size - h.size + 1, np.float64) if want_corr else None
    _call("mdm_xcorr_peak", device, _p(r), r.size, _p(h), h.size, _p(corr), _p(idx), _p(peak))
    return int(idx[0]), float(peak[0]), corr


def carrier_recovery(syms, init_phase, init_freq, alpha, kind, device=0):
    """The carrier loop over every row of syms [C, n] (complex128): (out [C, n],
    final [C, 2] = phase, freq).  Parameters per row, or scalars (mdm_carrier)."""
    s = np.asarray(syms)
    if s.ndim != 2:
        raise ValueError(f"syms has shape {s.shape}, expected (candidates, symbols)")
    s = np.ascontiguousarray(s.astype(np.complex128, copy=False))
    ph, fr, al, kd = _carrier_params(s.shape[0], init_phase, init_freq, alpha, kind)
    out = np.empty(s.shape, np.complex128)
    fin = np.empty((s.shape[0], 2), np.float64)
    if s.shape[0]:
        _call("mdm_carrier", device, _p(s), s.shape[0], s.shape[1], _p(ph), _p(fr), _p(al), _p(kd), _p(out), _p(fin))
    return out, fin


def mix_device(sig, w, fs, dc=None, i0=0, out=None, stream=None):
    out = _out(out, sig, sig.numel(), "complex128")
    dcv = _dc(dc)
    _call("mdm_mix_dev", _ordinal(sig), _p(sig), _f64(sig), sig.numel(), int(i0), _p(dcv), float(w), float(fs), _p(out),
          _n.stream_ptr(stream))
    return out


def _rx_scratch(n_out, scratch, like):
    return _out(scratch, like, 2 * -(-n_out // _RX_TILE), "int64")


def burst_find_device(sig, preamble_len, win=1000, dc=None, smooth=None, result=None, scratch=None, stream=None):
    """Stream-ordered; returns the int64[2] result record (burst_result decodes it)."""
    _check_burst(sig.numel(), win, preamble_len)
    result = _out(result, sig, 2, "int64")
    scratch = _rx_scratch(sig.numel(), scratch, sig)
    dcv = _dc(dc)
    _call("mdm_burst_find_dev", _ordinal(sig), _p(sig), _f64(sig), sig.numel(), _p(dcv), int(win), int(preamble_len),
          _p(smooth), _p(result), _p(scratch), _n.stream_ptr(stream))
    return result


def burst_result(result):
    """(burst_start, max smoothed power) of a burst_find_device record (synchronises)."""
    r = result.cpu().numpy()
    return int(r[0]), float(r[1:].view(np.float64)[0])


def xcorr_peak_device(region, wave, corr=None, result=None, scratch=None, stream=None):
    """Stream-ordered; returns the int64[2] result record (xcorr_result decodes it)."""
    import torch
    _check_xcorr(region.numel(), wave.numel())
    if region.dtype != torch.complex128 or wave.dtype != torch.complex128:
        raise ValueError("xcorr_peak_device takes complex128 tensors")
    result = _out(result, region, 2, "int64")
    scratch = _rx_scratch(region.numel() - wave.numel() + 1, scratch, region)
    _call("mdm_xcorr_peak_dev", _ordinal(region), _p(region), region.numel(), _p(wave), wave.numel(), _p(corr),
          _p(result), _p(scratch), _n.stream_ptr(stream))
    return result


def xcorr_result(result):
    """(argmax, peak) of an xcorr_peak_device record (synchronises)."""
    r = result.cpu().numpy()
    return int(r[1]), float(r[:1].view(np.float64)[0])


def carrier_recovery_device(syms, init_phase, init_freq, alpha, kind, out=None, final=None, stream=None):
    """syms: contiguous complex128 [C, n] on the GPU; parameters are host values
    (scalars or [C]), uploaded here.  Returns (out [C, n], final [C, 2])."""
    import torch
    if syms.dim() != 2 or syms.dtype != torch.complex128 or not syms.is_contiguous():
        raise ValueError("syms must be a contiguous complex128 tensor of shape (candidates, symbols)")
    C, n = syms.shape
    ph, fr, al, kd = (torch.from_numpy(a).to(syms.device) for a in _carrier_params(C, init_phase, init_freq, alpha, kind))
    out = _out(out, syms, (C, n), "complex128")
    final = _out(final, syms, (C, 2), "float64")
    if C:
        _call("mdm_carrier_dev", _ordinal(syms), _p(syms), C, n, _p(ph), _p(fr), _p(al), _p(kd), _p(out), _p(final),
              _n.stream_ptr(stream))
    return out, final


# ---------------------------------------------------------------- filter design (host) --------
def _rrc_taps(sps, alpha=0.35, ntaps=101):
    """sdr_modem.py:77-91 / test_sdr_with_coding.py:110-123: the same scalar
    expressions per tap (so the same rounding), normalised by np.linalg.norm."""
    h = np.zeros(ntaps)
    offs = np.arange(ntaps) - (ntaps - 1) / 2
    for i, t in enumerate(offs / sps):
        if t == 0:
            h[i] = 1 - alpha + 4 * alpha / np.pi
            continue
        if abs(abs(t) - 1 / (4 * alpha)) < 1e-8:
            h[i] = alpha / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / 4 / alpha) +
                                         (1 - 2 / np.pi) * np.cos(np.pi / 4 / alpha))
            continue
        den = np.pi * t * (1 - (4 * alpha * t) ** 2)
        if abs(den) > 1e-8:
            h[i] = (np.sin(np.pi * t * (1 - alpha)) + 4 * alpha * t * np.cos(np.pi * t * (1 + alpha))) / den
    return h / np.linalg.norm(h)


def rrc_taps(sps, alpha=0.35, ntaps=101):
    """test_sdr_with_coding.py:110-123."""
    return _rrc_taps(sps, alpha, ntaps)


def rrcosfilter(N, alpha, Ts, Fs):
    """modulators.py:19-47: int(N*Fs)|1 taps, the same per-tap expressions,
    normalised by sqrt(sum(h**2))."""
    n = int(N * Fs) | 1
    t_all = (np.arange(n) - (n - 1) / 2) * (1.0 / float(Fs))
    h = np.zeros(len(t_all), dtype=float)
    for i in range(n):
        t = t_all[i]
        if t == 0.0:
            h[i] = 1.0 - alpha + (4 * alpha / np.pi)
        elif alpha != 0 and abs(t) == Ts / (4 * alpha):
            h[i] = (alpha / np.sqrt(2)) * (((1 + 2 / np.pi) * (np.sin(np.pi / (4 * alpha)))) +
                                           ((1 - 2 / np.pi) * (np.cos(np.pi / (4 * alpha)))))
        else:
            den = 1 - (4 * alpha * t / Ts) ** 2
            if abs(den) < 1e-10:
                den = 1e-10
            h[i] = (np.sin(np.pi * t / Ts * (1 - alpha)) + 4 * alpha * t / Ts * np.cos(np.pi * t / Ts * (1 + alpha))) \
                / (np.pi * t / Ts * den)
    return h / np.sqrt(np.sum(h ** 2))


def _same_conv_up(syms, sps, taps, device):
    """np.convolve(up, taps, 'same') with up = zeros(len*sps, complex64), up[::sps] = syms."""
    s = np.asarray(syms)
    n_up = len(s) * sps
    if n_up == 0:
        raise ValueError("a cannot be empty")
    s = np.ascontiguousarray(s.astype(np.complex64).ravel())
    L = len(taps)
    return fir(s, taps, up=sps, down=1, offset=(min(n_up, L) - 1) // 2, n_out=max(n_up, L), device=device)


def upsample_filter(syms, sps, taps, device=0):
    """test_sdr_with_coding.py:125-128."""
    return _same_conv_up(syms, sps, taps, device)


# ---------------------------------------------------------------- IQ files ------------------
def save_iq(sig, fname, device=0):
    """test_sdr_with_coding.py:228-233 / sdr_modem.py:329-335."""
    iq_quantize(sig, device).tofile(fname)


def load_iq(fname, device=0):
    """test_sdr_with_coding.py:235-240 / sdr_modem.py:337-342."""
    return iq_dequantize(np.fromfile(fname, dtype=np.uint8), device)


# ---------------------------------------------------------------- Gray family ---------------
GRAY2, GRAY3, GRAY4 = D.GRAY2, D.GRAY3, D.GRAY4
_INV = {k: [g.index(i) for i in range(len(g))] for k, g in ((2, GRAY2), (3, GRAY3), (4, GRAY4))}

_TABLES = {}


def _gray_table(mod):
    t = _TABLES.get(("gray", mod))
    if t is None:
        t = _TABLES[("gray", mod)] = D.constellation(mod)   # the reference mappers over every label
    return t


def _loop_bits(bits):
    """np.array(list of Python ints) of the reference's per-symbol loops: int64,
    or float64 when empty."""
    return bits.astype(np.int64) if bits.size else np.array([])


def bpsk_mod(bits, device=0):
    """test_sdr_with_coding.py:25-26 / sdr_modem.py:101-102 (1 -> +1, 0 -> -1)."""
    return map_bits(bits, 1, _gray_table("BPSK"), device)


def bpsk_demod(syms, device=0):
    """test_sdr_with_coding.py:28-29 / sdr_modem.py:104-105."""
    return hard_demod(syms, GT0, 1, device=device).astype(int)


def qpsk_mod(bits, device=0):
    """test_sdr_with_coding.py:31-37 / sdr_modem.py:107-112 (complex128)."""
    return map_bits(bits, 2, _gray_table("QPSK"), device)


def qpsk_demod(syms, device=0):
    """test_sdr_with_coding.py:39-43 / sdr_modem.py:114-118."""
    return hard_demod(syms, QPSK, 2, device=device).astype(int)


def psk8_mod(bits, device=0):
    """test_sdr_with_coding.py:45-57 / sdr_modem.py:120-130."""
    return map_bits(bits, 3, _gray_table("8PSK"), device)


def psk8_demod(syms, device=0):
    """test_sdr_with_coding.py:59-70 / sdr_modem.py:132-140 (int(NaN) raises)."""
    return _loop_bits(hard_demod(syms, PSK8, 3, labels=_INV[3], nan_raises=True, device=device))


def _qam_demod(syms, k, scale, device):
    return _loop_bits(hard_demod(syms, QAM_AXIS, 2 * k, labels=_INV[k], scale=scale, device=device))


def qam16_mod(bits, device=0):
    """test_sdr_with_coding.py:72-86 / sdr_modem.py:142-154."""
    return map_bits(bits, 4, _gray_table("16QAM"), device)


def qam16_demod(syms, device=0):
    """test_sdr_with_coding.py:88-100 / sdr_modem.py:156-166."""
    return _qam_demod(syms, 2, np.sqrt(10), device)


MODULATIONS = {
    'BPSK': {'mod': bpsk_mod, 'demod': bpsk_demod, 'bps': 1, 'order': 2, 'alpha': 0.02},
    'QPSK': {'mod': qpsk_mod, 'demod': qpsk_demod, 'bps': 2, 'order': 4, 'alpha': 0.015},
    '8PSK': {'mod': psk8_mod, 'demod': psk8_demod, 'bps': 3, 'order': 8, 'alpha': 0.012},
    '16QAM': {'mod': qam16_mod, 'demod': qam16_demod, 'bps': 4, 'order': 16, 'alpha': 0.006},
}


class SDRModem:
    """sdr_modem.py:17-385, 523-664: mapping, hard demod, RRC shaping, IQ files,
    frame building and the burst-receive chain."""

    MODULATIONS = {
        'BPSK':   {'bps': 1, 'order': 2,   'alpha': 0.02,  'n_rot': 2, 'rot_step': np.pi},
        'QPSK':   {'bps': 2, 'order': 4,   'alpha': 0.015, 'n_rot': 4, 'rot_step': np.pi / 2},
        '8PSK':   {'bps': 3, 'order': 8,   'alpha': 0.01,  'n_rot': 8, 'rot_step': np.pi / 4},
        '16QAM':  {'bps': 4, 'order': 16,  'alpha': 0.008, 'n_rot': 4, 'rot_step': np.pi / 2},
        '64QAM':  {'bps': 6, 'order': 64,  'alpha': 0.005, 'n_rot': 4, 'rot_step': np.pi / 2},
        '256QAM': {'bps': 8, 'order': 256, 'alpha': 0.003, 'n_rot': 4, 'rot_step': np.pi / 2},
    }
    _QAM = {'16QAM': (2, 10), '64QAM': (3, 42), '256QAM': (4, 170)}

    def __init__(self, fc: float = 433e6, fs: float = 2e6, sps: int = 4, tx_gain: int = 47, rx_gain: int = 49,
                 device: int = 0):
        self.fc, self.fs, self.sps = fc, fs, sps
        self.tx_gain, self.rx_gain = tx_gain, rx_gain
        self.device = device
        self.rrc_taps = self._rrc_filter(sps)
        self.sync_bits = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0] * 10)
        self._sync_syms = None
        self._init_gray_tables()

    @property
    def sync_syms(self):
        if self._sync_syms is None:
            self._sync_syms = self._bpsk_mod(self.sync_bits)
        return self._sync_syms

    def _init_gray_tables(self):                     # :66-75
        self.gray2, self.gray3, self.gray4 = list(GRAY2), list(GRAY3), list(GRAY4)
        self.inv_gray2, self.inv_gray3, self.inv_gray4 = list(_INV[2]), list(_INV[3]), list(_INV[4])

    def _rrc_filter(self, sps: int, alpha: float = 0.35, ntaps: int = 101) -> np.ndarray:   # :77-91
        return _rrc_taps(sps, alpha, ntaps)

    def _upsample_filter(self, syms: np.ndarray) -> np.ndarray:                            # :93-97
        return _same_conv_up(syms, self.sps, self.rrc_taps, self.device)

    def _map(self, bits, mod):
        return map_bits(bits, self.MODULATIONS[mod]['bps'], _gray_table(mod), self.device)

    def _bpsk_mod(self, bits):
        return self._map(bits, 'BPSK')

    def _qpsk_mod(self, bits):
        return self._map(bits, 'QPSK')

    def _psk8_mod(self, bits):
        return self._map(bits, '8PSK')

    def _qam16_mod(self, bits):
        return self._map(bits, '16QAM')

    def _qam64_mod(self, bits):
        return self._map(bits, '64QAM')

    def _qam256_mod(self, bits):
        return self._map(bits, '256QAM')

    def _bpsk_demod(self, syms):
        return hard_demod(syms, GT0, 1, device=self.device).astype(int)

    def _qpsk_demod(self, syms):
        return hard_demod(syms, QPSK, 2, device=self.device).astype(int)

    def _psk8_demod(self, syms):
        return _loop_bits(hard_demod(syms, PSK8, 3, labels=_INV[3], nan_raises=True, device=self.device))

    def _qam_demod(self, syms, mod):
        k, s = self._QAM[mod]
        return _qam_demod(syms, k, np.sqrt(s), self.device)

    def _qam16_demod(self, syms):
        return self._qam_demod(syms, '16QAM')

    def _qam64_demod(self, syms):
        return self._qam_demod(syms, '64QAM')

    def _qam256_demod(self, syms):
        return self._qam_demod(syms, '256QAM')

    def modulate(self, bits: np.ndarray, modulation: str = 'QPSK') -> np.ndarray:          # :222-243
        if modulation not in self.MODULATIONS:
            raise ValueError(f"Unknown modulation: {modulation}")
        return self._map(bits, modulation)

    def demodulate(self, symbols: np.ndarray, modulation: str = 'QPSK') -> np.ndarray:     # :245-266
        f = {'BPSK': self._bpsk_demod, 'QPSK': self._qpsk_demod, '8PSK': self._psk8_demod,
             '16QAM': self._qam16_demod, '64QAM': self._qam64_demod, '256QAM': self._qam256_demod}
        if modulation not in f:
            raise ValueError(f"Unknown modulation: {modulation}")
        return f[modulation](symbols)

    def _save_iq(self, sig: np.ndarray, filename: str):                                    # :329-335
        save_iq(sig, filename, self.device)

    def _load_iq(self, filename: str) -> np.ndarray:                                       # :337-342
        return load_iq(filename, self.device)

    # ---- burst-receive chain (:270-325, 346-385, 523-664) ----
    def _estimate_freq_offset(self, sig: np.ndarray) -> float:                             # :270-280
        """Host numpy, exactly the reference's expressions: one <= 65 536-point FFT
        of a preamble slice, off the hot path.  It stays on the host because an FFT
        on the GPU cannot be made bit-stable against numpy's pocketfft, and the
        estimate feeds every later step."""
        N = min(len(sig), 2 ** 16)
        sig = sig[:N]
        win = np.hanning(N)
        fft = np.fft.fft(sig * win)
        freqs = np.fft.fftfreq(N, 1 / self.fs)
        mag = np.abs(fft)
        mag[:N // 100] = 0
        mag[-N // 100:] = 0
        return freqs[np.argmax(mag)]

    def _correct_freq(self, sig: np.ndarray, f_offset: float) -> np.ndarray:               # :282-285
        return mix(sig, (-1j * 2 * np.pi * f_offset).imag, self.fs, device=self.device)

    def _carrier_recovery_bpsk(self, syms: np.ndarray, alpha: float = 0.03):               # :287-300
        """(out, phase, freq).  The loop runs in complex128 / f64 whatever the
        input's dtype (the reference's arithmetic follows a complex64 input's)."""
        out, fin = carrier_recovery(np.asarray(syms).reshape(1, -1), 0.0, 0.0, alpha, CR_BPSK, self.device)
        return out[0], fin[0, 0], fin[0, 1]

    @staticmethod
    def _detector(modulation):
        if modulation == 'BPSK':
            return CR_BPSK
        return CR_QUAD if modulation in ('QPSK', '16QAM', '64QAM', '256QAM') else CR_PSK8   # else: 8PSK (:317)

    def _carrier_recovery_data(self, syms: np.ndarray, init_phase: float, init_freq: float, modulation: str,
                               alpha: float) -> np.ndarray:                                # :302-325
        return carrier_recovery(np.asarray(syms).reshape(1, -1), init_phase, init_freq, alpha,
                                self._detector(modulation), self.device)[0][0]

    def _sync_bits_for(self, modulation):                                                  # :364-368, :561-565
        if self.MODULATIONS[modulation]['order'] >= 64:
            return np.array([1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0] * 15)
        return self.sync_bits

    def build_frame(self, data_bits: np.ndarray, modulation: str = 'QPSK', n_repeats: int = 20) -> np.ndarray:
        """:346-385: pad | CW preamble | RRC-shaped (sync, data) | pad, tiled."""
        preamble = np.ones(int(0.01 * self.fs), dtype=np.complex64)
        sync_syms = self._bpsk_mod(self._sync_bits_for(modulation))
        data_syms = self.modulate(data_bits, modulation)
        frame_wave = self._upsample_filter(np.concatenate([sync_syms, data_syms]))
        full_sig = np.concatenate([preamble, frame_wave])
        pad = np.zeros(int(0.02 * self.fs), dtype=np.complex64)
        return np.tile(np.concatenate([pad, full_sig, pad]), n_repeats)

    def _process_received(self, rx_raw: np.ndarray, modulation: str, n_expected_bits: int):   # :523-664
        """(bits, stats) of a captured burst, with the reference's stats keys and
        error strings.  The capture is uploaded once; DC removal + power detection,
        frequency correction, matched filter, sync search and both carrier loops
        (every timing offset and sync rotation in one call each) run on the GPU
        without leaving it.  On the host: np.mean of the capture, the preamble FFT
        (_estimate_freq_offset), and the candidate choice and normalisation of
        :617-651 on the few hundred recovered symbols, in the reference's own
        expressions.  The demodulate() calls the reference makes inside its
        rotation loop and discards are not made."""
        import torch
        x = _syms_c(rx_raw)
        stats = {'success': False, 'n_samples': len(x)}
        dev = torch.device('cuda', self.device)
        mean = np.mean(x)                                   # :529, the signal's precision
        preamble_len = int(0.01 * self.fs)
        d_x = torch.from_numpy(x).to(dev)
        burst_start, _ = burst_result(burst_find_device(d_x, preamble_len, 1000, dc=mean))
        if burst_start < 0:
            stats['error'] = 'Could not find burst'
            return None, stats
        stats['burst_start'] = burst_start

        preamble_rx = x[burst_start:burst_start + preamble_len] - mean
        f_offset = self._estimate_freq_offset(preamble_rx)
        stats['freq_offset'] = f_offset
        d_corr = mix_device(d_x, (-1j * 2 * np.pi * f_offset).imag, self.fs, dc=mean)
        L = len(self.rrc_taps)
        d_filt = fir_device(d_corr, self.rrc_taps, 1, 1, (min(len(x), L) - 1) // 2, max(len(x), L))

        sync_bits = self._sync_bits_for(modulation)
        sync_syms = self._bpsk_mod(sync_bits)
        d_wave = torch.from_numpy(self._upsample_filter(sync_syms)).to(dev)
        search_start = burst_start + preamble_len - 100
        search_end = min(d_filt.numel(), burst_start + int(0.5 * self.fs))
        peak_idx, peak = xcorr_result(xcorr_peak_device(d_filt[search_start:search_end], d_wave))
        sync_start = search_start + peak_idx
        stats['sync_peak'] = np.float64(peak)
        stats['sync_start'] = sync_start

        mod_cfg = self.MODULATIONS[modulation]
        bps = mod_cfg['bps']
        n_sync = len(sync_syms)
        n_data_syms = (n_expected_bits + bps - 1) // bps
        total_syms = n_sync + n_data_syms
        frame_samples = total_syms * self.sps + self.sps * 4
        if sync_start + frame_samples > d_filt.numel():
            stats['error'] = 'Frame past buffer'
            return None, stats
        d_frame = d_filt[sync_start:sync_start + frame_samples]

        # every timing offset through the sync loop in one call
        offsets = [o for o in range(self.sps) if d_frame[o::self.sps].numel() >= total_syms]
        if not offsets:
            stats['error'] = 'Could not decode'
            return None, stats
        d_syms = torch.stack([d_frame[o::self.sps][:total_syms] for o in offsets])
        d_sync, d_fin = carrier_recovery_device(d_syms[:, :n_sync].contiguous(), 0.0, 0.0, 0.03, CR_BPSK)
        sync_rec_all, fin = d_sync.cpu().numpy(), d_fin.cpu().numpy()
        tests = []
        for k in range(len(offsets)):
            sync_rec = sync_rec_all[k]
            pwr = np.mean(np.abs(sync_rec) ** 2)
            if pwr > 0:
                sync_rec = sync_rec / np.sqrt(pwr)
            for sync_rot in range(2):
                tests.append(sync_rec * np.exp(1j * sync_rot * np.pi))
        sync_rx = hard_demod(np.concatenate(tests), GT0, 1, device=self.device).astype(int).reshape(len(tests), n_sync)

        # every (offset, rotation) that passes the sync check through the data loop in one call
        cand = []
        for k in range(len(offsets)):
            for sync_rot in range(2):
                sync_ber = np.mean(sync_rx[2 * k + sync_rot] != sync_bits)
                if sync_ber > 0.2:
                    continue
                cand.append((k, sync_ber, fin[k, 0] + sync_rot * np.pi, fin[k, 1]))
        if not cand:
            stats['error'] = 'Could not decode'
            return None, stats
        rows = torch.tensor([c[0] for c in cand], device=dev)
        d_data, _ = carrier_recovery_device(d_syms[rows, n_sync:].contiguous(), [c[2] for c in cand],
                                            [c[3] for c in cand], mod_cfg['alpha'], self._detector(modulation))
        data_all = d_data.cpu().numpy()

        best_data_rx = None
        best_sync_ber = 1.0
        for j, (_, sync_ber, _, _) in enumerate(cand):
            data_rec = data_all[j]
            pwr = np.mean(np.abs(data_rec) ** 2)
            if pwr > 0:
                data_rec = data_rec / np.sqrt(pwr)
            for rot in range(mod_cfg['n_rot']):
                if sync_ber < best_sync_ber:               # holds at the first rotation only (:649-651)
                    best_sync_ber = sync_ber
                    best_data_rx = data_rec * np.exp(1j * rot * mod_cfg['rot_step'])
        if best_data_rx is None:
            stats['error'] = 'Could not decode'
            return None, stats

        data_bits_rx = self.demodulate(best_data_rx, modulation)
        stats['success'] = True
        stats['sync_ber'] = best_sync_ber
        stats['rx_symbols'] = best_data_rx
        return data_bits_rx[:n_expected_bits], stats


# ---------------------------------------------------------------- natural family -------------
class Modulator:
    """modulators.py:50-199: natural-label mappers, argmin QAM demods, RRC
    pulse shaping (scipy upfirdn) and matched filtering."""

    def __init__(self, samples_per_symbol=8, bt=0.3, rrc_alpha=0.35, rrc_span=6, device=0):
        self.sps = int(samples_per_symbol)
        self.bt = float(bt)
        self.rrc_alpha = rrc_alpha
        self.rrc_span = rrc_span
        self.device = device
        self.rrc_filter = rrcosfilter(self.rrc_span, self.rrc_alpha, 1, self.sps)
        self.filter_delay = (len(self.rrc_filter) - 1) // 2
        self._tables = {}

    # ---- pulse shaping (:67-113)
    def apply_pulse_shaping(self, symbols):
        """upfirdn(h, syms, up=sps): (len-1)*sps + len(h) samples, complex128."""
        syms = np.array(symbols, dtype=np.complex64).ravel()
        if syms.size == 0:
            raise ValueError("x must be at least 1-D with at least 1 element")
        L = len(self.rrc_filter)
        return fir(syms, self.rrc_filter, up=self.sps, down=1, offset=0, n_out=(syms.size - 1) * self.sps + L,
                   device=self.device)

    def matched_filter(self, samples):
        """full convolution with h, then [2*delay::sps]."""
        x = np.asarray(samples)
        L = len(self.rrc_filter)
        n_full = x.size + L - 1
        start = 2 * self.filter_delay
        if start >= n_full:
            return np.array([], dtype=np.complex64)
        y = fir(x, self.rrc_filter, up=1, down=self.sps, offset=start, n_out=-(-(n_full - start) // self.sps),
                device=self.device)
        return y if np.iscomplexobj(x) else y.real.copy()

    # ---- tables: the reference expressions over every label
    def _table(self, name):
        t = self._tables.get(name)
        if t is None:
            if name == 'bpsk':
                t = (2 * np.arange(2) - 1).astype(np.complex64)                          # :119-120
            elif name == 'qpsk':
                b = np.array([[i >> 1, i & 1] for i in range(4)])
                t = ((1 - 2 * b[:, 0]) + 1j * (1 - 2 * b[:, 1])) / np.sqrt(2)           # :125-131
            elif name == '8psk':
                t = np.exp(1j * 2 * np.pi * np.arange(8) / 8)                             # :139-145
            else:
                t = self._qam_const(int(name[3:]))[0]                                     # :174-197
            self._tables[name] = t = np.ascontiguousarray(t)
        return t

    def _qam_const(self, M):                                                              # :157-163
        m = int(np.sqrt(M))
        axis = np.arange(-m + 1, m, 2)
        xv, yv = np.meshgrid(axis, axis)
        c = xv.flatten() + 1j * yv.flatten()
        c /= np.sqrt(np.mean(np.abs(c) ** 2))
        return c, axis

    def mod_bpsk(self, bits):
        return map_bits(bits, 1, self._table('bpsk'), self.device)

    def demod_bpsk(self, symbols):
        return hard_demod(symbols, GT0, 1, device=self.device).astype(int)

    def mod_qpsk(self, bits):
        return map_bits(bits, 2, self._table('qpsk'), self.device)

    def demod_qpsk(self, symbols):
        return hard_demod(symbols, QPSK, 2, device=self.device).astype(int)

    def mod_8psk(self, bits):
        return map_bits(bits, 3, self._table('8psk'), self.device)

    def demod_8psk(self, symbols):
        """astype(int) of a NaN angle is INT64_MIN on x86, and % 8 -> 0."""
        return _loop_bits(hard_demod(symbols, PSK8, 3, nan_raises=False, device=self.device))

    def _demod_qam_generic(self, symbols, M):
        k = int(np.log2(M))
        return _loop_bits(hard_demod(symbols, ARGMIN, k, cons=self._qam_const(M)[0], device=self.device))

    def mod_16qam(self, bits):
        return map_bits(bits, 4, self._table('qam16'), self.device)

    def demod_16qam(self, symbols):
        return self._demod_qam_generic(symbols, 16)

    def mod_64qam(self, bits):
        return map_bits(bits, 6, self._table('qam64'), self.device)

    def demod_64qam(self, symbols):
        return self._demod_qam_generic(symbols, 64)
