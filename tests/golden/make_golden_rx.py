#!/usr/bin/env python3
"""Generate the committed golden vectors of the burst-receive chain
(sdr_modem.py:270-325, 346-385, 523-664): frequency correction, power
detection, sync correlation, both carrier loops and _process_received.

TEST INFRASTRUCTURE ONLY.  Runs in the build container, where the read-only
reference checkout lives at /root/reference; it imports the reference's
``sdr_modem`` module unmodified and records inputs and outputs as plain
arrays in ``rx.npz``.  The intermediate arrays of ``_process_received`` are
not restated here: the reference's own calls (np.convolve, scipy's correlate,
_correct_freq, _estimate_freq_offset, the two carrier loops) are wrapped with
recorders while the unmodified method runs, so every array is what the
reference itself computed.

Captures: fs = 200 kHz (preamble 2 000 samples), one burst of
build_frame(bits, mod, n_repeats=1) with 2 500 / 1 200 samples of padding cut from
its head / tail, through a frequency offset, a constant phase, AWGN from a seeded
default_rng and the uint8 quantisation that _load_iq reads back.  The
frequency offset is F0 = 5.3 kHz, not a few hundred Hz: _estimate_freq_offset
blanks the first and last N // 100 FFT bins (+-2 kHz at this fs, +-20 kHz at
2 MHz), so the reference itself cannot decode a burst whose offset lies inside
that band (checked below: main() asserts that a 300 Hz capture fails or
decodes with errors, so the choice is visible if the reference ever changes).

Every property a test relies on is asserted here on the reference's own
arrays; a capture that misses one is an error, not a silently weaker fixture.

Usage:  python tests/golden/make_golden_rx.py
"""
import os
import sys
import tempfile

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
FS = 200e3
F0 = 5300.0
PHI = 0.7
SIGMA = 0.01          # AWGN per component; symbols have amplitude ~0.55 after shaping
CUT_HEAD, CUT_TAIL = 2500, 1200   # padding samples dropped from the 4 000 build_frame adds at each end
N_BITS = {"QPSK": 240, "8PSK": 240, "16QAM": 240}


def _import():
    try:
        from scipy.signal import correlate  # noqa: F401
    except Exception as e:   # noqa: BLE001
        raise SystemExit(f"scipy.signal.correlate is not importable ({e}); the golden correlation is scipy's own "
                         "and no other correlator may stand in for it")
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import sdr_modem as SM
    return SM


def make_capture(m, rng, bits, mod, f0, d):
    """uint8 IQ file of one burst through the channel, read back by the reference's _load_iq."""
    tx = m.build_frame(bits, mod, n_repeats=1)[CUT_HEAD:-CUT_TAIL]
    t = np.arange(len(tx)) / m.fs
    x = tx * np.exp(1j * (2 * np.pi * f0 * t + PHI))
    x = x + SIGMA * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    x = x * (0.8 / np.max(np.abs(x)))
    raw = np.empty(2 * len(x), np.uint8)
    raw[0::2] = np.clip(np.round(x.real * 127.5 + 127.5), 0, 255)
    raw[1::2] = np.clip(np.round(x.imag * 127.5 + 127.5), 0, 255)
    f = os.path.join(d, "cap.iq")
    raw.tofile(f)
    return m._load_iq(f)


class Recorder:
    """Wraps callables; keeps (args, result) of every call by name."""

    def __init__(self):
        self.calls = {}

    def wrap(self, name, fn):
        def w(*a, **k):
            r = fn(*a, **k)
            self.calls.setdefault(name, []).append((a, k, r))
            return r
        return w


def run_recorded(SM, m, cap, mod, n_bits):
    rec = Recorder()
    saved_conv, saved_corr = np.convolve, SM.correlate
    for name in ("_correct_freq", "_estimate_freq_offset", "_carrier_recovery_bpsk", "_carrier_recovery_data"):
        setattr(m, name, rec.wrap(name, getattr(type(m), name).__get__(m)))
    np.convolve = rec.wrap("convolve", saved_conv)
    SM.correlate = rec.wrap("correlate", saved_corr)
    try:
        bits, stats = m._process_received(cap, mod, n_bits)
    finally:
        np.convolve, SM.correlate = saved_conv, saved_corr
        for name in ("_correct_freq", "_estimate_freq_offset", "_carrier_recovery_bpsk", "_carrier_recovery_data"):
            delattr(m, name)
    return bits, stats, rec.calls


sys.path.insert(0, os.path.dirname(OUT))
from rx_patterns import first_run  # noqa: E402  (tests/rx_patterns.py: the search as a sliding count)

QAM_AXIS = {"16QAM": (4, 10), "64QAM": (8, 42), "256QAM": (16, 170)}   # levels per axis, 1 / scale ** 2


def boundary_margin(syms, mod):
    """Smallest distance of a symbol from a decision boundary of the hard demodulator."""
    if mod == "BPSK":
        return np.min(np.abs(syms.real))
    if mod == "QPSK":
        return min(np.min(np.abs(syms.real)), np.min(np.abs(syms.imag)))
    if mod == "8PSK":
        q = np.angle(syms) / (np.pi / 4)
        return np.min(np.abs((q - np.floor(q)) - 0.5) * (np.pi / 4) * np.abs(syms))
    levels, s = QAM_AXIS[mod]
    x = np.concatenate([syms.real, syms.imag]) * np.sqrt(s)
    edges = np.arange(-(levels - 2), levels - 1, 2.0)      # 16QAM: -2, 0, 2; 64QAM: -6 .. 6
    return np.min(np.abs(x[:, None] - edges[None, :])) / np.sqrt(s)


def halfway_symbol():
    """r * exp(j pi/8) whose np.angle / (pi/4) is exactly 0.5 and whose arctan2 is as far from a
    rounding boundary as a scan finds, so a correctly rounded atan2 and one with a small error
    return the same double.  round-half-even sends 0.5 to 0, round-half-up to 1."""
    best = None
    for r in np.linspace(0.5, 1.5, 4001):
        z = complex(r * np.cos(np.pi / 8), r * np.sin(np.pi / 8))
        a = np.angle(z)
        if a / (np.pi / 4) != 0.5:
            continue
        exact = np.arctan2(np.longdouble(z.imag), np.longdouble(z.real))
        off = abs(float((exact - np.longdouble(a)) / np.longdouble(np.spacing(a))))
        if best is None or off < best[0]:
            best = (off, z)
    assert best is not None and best[0] < 0.05, best
    return best[1]


def main():
    SM = _import()
    from scipy.signal import correlate
    rng = np.random.default_rng(20260419)
    out = {"fs": np.float64(FS)}
    m = SM.SDRModem(fs=FS)
    pre = int(0.01 * FS)

    with tempfile.TemporaryDirectory() as d:
        # the blanked FFT bins: the reference does not decode a 300 Hz offset cleanly
        b300 = rng.integers(0, 2, 240)
        bits, stats = m._process_received(make_capture(m, rng, b300, "QPSK", 300.0, d), "QPSK", 240)
        assert bits is None or np.any(bits != b300), "a 300 Hz offset decodes: use it, as a capture would have"

        for mod, nb in N_BITS.items():
            tx_bits = rng.integers(0, 2, nb)
            cap = make_capture(m, rng, tx_bits, mod, F0, d)
            bits, stats, calls = run_recorded(SM, m, cap, mod, nb)
            assert stats["success"], (mod, stats)
            assert np.array_equal(bits, tx_bits), (mod, "the fixture must decode without errors")
            k = f"_{mod}"
            out["tx_bits" + k] = tx_bits
            out["cap" + k] = cap
            assert cap.dtype == np.complex64

            # power detection: the first np.convolve call
            (power, kern), _, smooth = calls["convolve"][0]
            assert len(kern) == 1000 and power.dtype == np.float32
            out["power_smooth" + k] = smooth
            out["burst_start" + k] = np.int64(stats["burst_start"])
            thr = np.max(smooth) * 0.3
            for s in (1.0, 1 - 1e-6, 1 + 1e-6):
                assert first_run(smooth > thr * s, pre) == stats["burst_start"], (mod, s)

            # frequency correction
            (rx, f_off), _, rx_corr = calls["_correct_freq"][0]
            assert rx.dtype == np.complex64 and np.array_equal(rx, cap - np.mean(cap))
            assert f_off == stats["freq_offset"]
            out["freq_offset" + k] = np.float64(f_off)
            out["rx_corrected" + k] = rx_corr

            # sync search
            (region, wave), _, c = calls["correlate"][0]
            corr = np.abs(c)
            peak_idx = int(np.argmax(corr))
            assert corr[peak_idx] == stats["sync_peak"]
            far = np.ones(len(corr), bool)
            far[max(0, peak_idx - m.sps):peak_idx + m.sps + 1] = False
            # the sync word repeats every 16 symbols, so the reference's correlation has side peaks of
            # 144/160 = 0.9 x peak (plus what the data adds) at +-64 samples whatever the capture: the
            # runner-up is bounded at 0.95 x peak, still eight orders above any rounding difference
            assert np.max(corr[far]) < 0.95 * corr[peak_idx], mod
            assert len(corr) > 2 * 1024, "the region must span three workgroups of the correlator"
            out["region" + k] = np.ascontiguousarray(region)
            out["sync_wave" + k] = wave
            out["corr" + k] = corr
            out["peak_idx" + k] = np.int64(peak_idx)
            out["sync_peak" + k] = np.float64(stats["sync_peak"])
            out["sync_start" + k] = np.int64(stats["sync_start"])

            # carrier loops: one call per timing offset (sync) and per passing candidate (data)
            cb = calls["_carrier_recovery_bpsk"]
            out["cr_sync_in" + k] = np.stack([a[0] for a, _, _ in cb])
            out["cr_sync_out" + k] = np.stack([r[0] for _, _, r in cb])
            out["cr_sync_final" + k] = np.array([[r[1], r[2]] for _, _, r in cb])
            cd = calls["_carrier_recovery_data"]
            out["cr_data_in" + k] = np.stack([a[0] for a, _, _ in cd])
            out["cr_data_par" + k] = np.array([[a[1], a[2], a[4]] for a, _, _ in cd])   # phase, freq, alpha
            assert all(a[3] == mod for a, _, _ in cd)
            out["cr_data_out" + k] = np.stack([r for _, _, r in cd])

            # end to end
            out["bits" + k] = np.asarray(bits)
            out["sync_ber" + k] = np.float64(stats["sync_ber"])
            out["rx_symbols" + k] = stats["rx_symbols"]
            assert boundary_margin(stats["rx_symbols"], mod) > 1e-6, mod

            # truncated capture: the sync is found, the frame runs past the buffer
            if mod == "QPSK":
                n_sym = 160 + nb // 2
                cut = int(stats["sync_start"]) + n_sym * m.sps + m.sps * 4 - 8
                b2, s2 = m._process_received(cap[:cut], mod, nb)
                assert b2 is None and s2["error"] == "Frame past buffer", s2
                out["trunc_len"] = np.int64(cut)
                out["trunc_burst_start"] = np.int64(s2["burst_start"])
                out["trunc_sync_start"] = np.int64(s2["sync_start"])
                b3, s3 = m._process_received(np.zeros(4096, np.complex64), mod, nb)
                assert b3 is None and s3["error"] == "Could not find burst" and set(s3) == {"success", "n_samples",
                                                                                            "error"}

    # ---- correlator shapes: scipy on slices of the QPSK region ------------------------------
    region, wave = out["region_QPSK"], out["sync_wave_QPSK"]
    assert len(wave) == 640
    for name, nr, w in (("one", 640, wave), ("p641", 641, wave), ("p703", 703, wave), ("w17", 2000, wave[300:317])):
        out["xc_" + name] = np.abs(correlate(region[:nr], w, mode="valid"))

    # ---- carrier loop, data form, on a batch: BPSK / QPSK / 8PSK by turns ----------------------
    # 65 streams of 40 symbols with different parameters each; stream 0 (BPSK) starts with a
    # symbol whose real part is 0, stream 1 (QPSK) with one whose imaginary part is 0, stream 2
    # (8PSK) with one exactly halfway between two constellation angles.
    mods = ("BPSK", "QPSK", "8PSK")
    C, n = 65, 40
    syms = np.empty((C, n), np.complex128)
    par = np.empty((C, 3))
    res = np.empty((C, n), np.complex128)
    for c in range(C):
        bps = c % 3 + 1
        labels = np.array([list(map(int, format(i, f"0{bps}b"))) for i in range(2 ** bps)]).ravel()
        const = m.modulate(labels, mods[c % 3]).astype(np.complex128)
        syms[c] = const[rng.integers(0, len(const), n)] * np.exp(1j * 0.1) \
            + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        par[c] = (0.0, 0.0, 0.03) if c < 3 else (rng.uniform(-0.3, 0.3), rng.uniform(-0.01, 0.01),
                                                    rng.uniform(0.005, 0.03))
    syms[0, 0] = 1j
    syms[1, 0] = 1.0
    syms[2, 0] = halfway_symbol()
    for c in range(C):
        res[c] = m._carrier_recovery_data(syms[c], par[c, 0], par[c, 1], mods[c % 3], par[c, 2])
    assert res[0, 0].real == 0 and res[1, 0].imag == 0
    assert np.angle(res[2, 0]) / (np.pi / 4) == 0.5
    out["crb_in"], out["crb_par"], out["crb_out"] = syms, par, res
    out["crb_kind"] = np.array([c % 3 for c in range(C)], np.int32)   # MDM_CR_BPSK / _QUAD / _PSK8 of each stream

    for k, v in out.items():
        v = np.asarray(v)
        assert v.dtype.kind in "cfiu" and v.dtype != object, k
        if v.dtype.kind == "c":
            assert v.dtype in (np.complex64, np.complex128), k
    path = os.path.join(OUT, "rx.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print("wrote", path, len(out), "arrays", size, "bytes")


if __name__ == "__main__":
    main()
