#!/usr/bin/env python3
"""Generate rx_more.npz: end-to-end captures of _process_received for the
modulations rx.npz does not hold -- BPSK (the BPSK detector of the data loop)
and 64QAM (the 240-symbol sync word of order >= 64, a 960-tap sync wave, and
the QPSK-style detector on a dense QAM).

TEST INFRASTRUCTURE ONLY.  Same method as make_golden_rx.py, whose make_capture
and boundary_margin are imported, not copied: the reference's ``sdr_modem``
module is imported unmodified in the build container, one burst per modulation
goes through the same channel (5.3 kHz offset, constant phase, seeded AWGN,
uint8 quantisation), and only the end-to-end inputs and results are recorded:
the capture, tx_bits, burst_start, freq_offset, sync_start, sync_peak, sync_ber,
rx_symbols, bits.  rx.npz is not touched.

256QAM: tried and left out.  Through this channel, and through the same channel
without noise, the reference decodes 240 bits of 256QAM with 1 to 13 bit errors
in 11 of 12 captures (seeds 0..5): the 30 data symbols are normalised by their
own mean power, which for so few symbols of 256 levels is off by more than the
spacing of the outer points.  main() repeats that trial and fails if it ever
turns out otherwise.  A 64QAM draw can fail in the reference the same way (40
symbols); the seed below is one whose draw decodes, which main() asserts.

Usage:  python tests/golden/make_golden_rx_more.py
"""
import os
import tempfile

import numpy as np

import make_golden_rx as R

MODS = {"BPSK": 240, "64QAM": 240}   # modulation -> n_expected_bits
SEED = 20261019                      # each modulation draws from default_rng([SEED, its index])
KEYS = ("burst_start", "freq_offset", "sync_start", "sync_peak", "sync_ber", "rx_symbols")


def try_256qam(m, d):
    """Bit errors of the reference on 256QAM captures of six seeds, noiseless ones included."""
    errs = []
    sigma = R.SIGMA
    try:
        for seed in range(6):
            for R.SIGMA in (sigma, 0.0):
                rng = np.random.default_rng(seed)
                tx_bits = rng.integers(0, 2, 240)
                bits, _ = m._process_received(R.make_capture(m, rng, tx_bits, "256QAM", R.F0, d), "256QAM", 240)
                errs.append(240 if bits is None else int(np.sum(bits != tx_bits)))
    finally:
        R.SIGMA = sigma
    return errs


def main():
    SM = R._import()
    m = SM.SDRModem(fs=R.FS)
    out = {"fs": np.float64(R.FS)}
    with tempfile.TemporaryDirectory() as d:
        errs = try_256qam(m, d)
        print("256QAM bit errors of the reference over 12 captures:", errs)
        assert sum(e > 0 for e in errs) >= 10, "256QAM decodes now: add it to MODS"
        for i, (mod, nb) in enumerate(MODS.items()):
            rng = np.random.default_rng([SEED, i])
            tx_bits = rng.integers(0, 2, nb)
            cap = R.make_capture(m, rng, tx_bits, mod, R.F0, d)
            bits, stats = m._process_received(cap, mod, nb)
            assert stats["success"], (mod, stats)
            assert np.array_equal(bits, tx_bits), (mod, "the fixture must decode without errors")
            margin = R.boundary_margin(stats["rx_symbols"], mod)
            assert margin > 1e-6, (mod, margin)
            assert cap.dtype == np.complex64
            k = f"_{mod}"
            out["cap" + k] = cap
            out["tx_bits" + k] = tx_bits
            out["bits" + k] = np.asarray(bits)
            for key in KEYS:
                out[key + k] = np.asarray(stats[key])
            print(mod, "burst_start", stats["burst_start"], "sync_start", stats["sync_start"], "sync_ber",
                  stats["sync_ber"], "boundary margin", margin)
    for k, v in out.items():
        assert v.dtype.kind in "cfiu" and v.dtype in (np.complex64, np.complex128, np.float64, np.int64), (k, v.dtype)
    path = os.path.join(R.OUT, "rx_more.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print("wrote", path, len(out), "arrays", size, "bytes")


if __name__ == "__main__":
    main()
