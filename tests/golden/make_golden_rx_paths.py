#!/usr/bin/env python3
"""Generate rx_paths.npz: two QPSK captures that take _process_received down the paths the
captures of rx.npz and rx_more.npz never take.

  nosync   a burst whose sync word is not the receiver's (the frame is built with 160 other
           bits in place of the sync word): the burst is found, the correlator returns some
           peak, every (timing offset, sync rotation) fails the sync check and the reference
           returns 'Could not decode'
  rot      a burst received half a turn off (constant phase PHI + pi): the BPSK sync loop locks
           on the inverted sync word, so every candidate that passes the sync check, the
           accepted one included, has sync_rot = 1 and starts the data loop at the sync loop's
           final phase + pi; more than one timing offset reaches the data loop

TEST INFRASTRUCTURE ONLY.  Same method as make_golden_rx.py, whose make_capture, recorder and
boundary_margin are imported, not copied: the reference's ``sdr_modem`` module is imported
unmodified in the build container and only inputs and results are recorded.  Every property a
test relies on is asserted here on the reference's own arrays, with margins that a rounding
difference cannot cross.  rx.npz and rx_more.npz are not touched; main() also asserts that the
captures of rx.npz already pass more than one timing offset into the data loop.

Usage:  python tests/golden/make_golden_rx_paths.py
"""
import os
import tempfile

import numpy as np

import make_golden_rx as R

SEED = 20261103
MOD, N_BITS = "QPSK", 240
TILE = 1024


def recorded(SM, m, cap):
    """run_recorded, with the sync check's hard decisions recorded as well."""
    rec = R.Recorder()
    m._bpsk_demod = rec.wrap("_bpsk_demod", type(m)._bpsk_demod.__get__(m))
    try:
        bits, stats, calls = R.run_recorded(SM, m, cap, MOD, N_BITS)
    finally:
        del m._bpsk_demod
    calls["_bpsk_demod"] = rec.calls["_bpsk_demod"]
    return bits, stats, calls


def check_front(m, stats, calls):
    """The exact results up to the sync search are robust: the burst start against the threshold,
    the correlation's peak against its runner-up."""
    pre = int(0.01 * m.fs)
    (_, kern), _, smooth = calls["convolve"][0]
    assert len(kern) == 1000
    thr = np.max(smooth) * 0.3
    for s in (1.0, 1 - 1e-6, 1 + 1e-6):
        assert R.first_run(smooth > thr * s, pre) == stats["burst_start"], s
    (_, _), _, c = calls["correlate"][0]
    corr = np.abs(c)
    peak_idx = int(np.argmax(corr))
    assert corr[peak_idx] == stats["sync_peak"]
    others = np.delete(corr, peak_idx)
    assert np.max(others) < (1 - 1e-6) * corr[peak_idx], (np.max(others), corr[peak_idx])


def sync_bers(m, calls):
    """Bit error rate of every (offset, rotation) of the sync check, in the reference's order, after
    asserting that no decision is within 1e-6 of its boundary."""
    demods = calls["_bpsk_demod"]
    assert len(demods) == 2 * len(calls["_carrier_recovery_bpsk"]) == 2 * m.sps
    bers = []
    for (syms,), _, bits in demods:
        assert np.min(np.abs(syms.real)) > 1e-6
        bers.append(float(np.mean(bits != m.sync_bits)))
    return np.array(bers).reshape(m.sps, 2)


def main():
    SM = R._import()
    m = SM.SDRModem(fs=R.FS)
    out = {"fs": np.float64(R.FS), "n_bits": np.int64(N_BITS)}

    # what the existing captures reach: two timing offsets in the data loop, rotation 0 only
    G = np.load(os.path.join(R.OUT, "rx.npz"), allow_pickle=False)
    for mod in ("QPSK", "8PSK", "16QAM"):
        par, fin = G[f"cr_data_par_{mod}"], G[f"cr_sync_final_{mod}"]
        assert len(set(par[:, 1])) >= 2, (mod, "one timing offset only")
        assert all(np.any((fin[:, 0] == p[0]) & (fin[:, 1] == p[1])) for p in par), (mod, "a sync_rot = 1 candidate")
        print(mod, "in rx.npz:", len(set(par[:, 1])), "timing offsets reach the data loop, all with sync_rot = 0")

    with tempfile.TemporaryDirectory() as d:
        # ---- nosync ---------------------------------------------------------------------------
        rng = np.random.default_rng([SEED, 0])
        tx_bits = rng.integers(0, 2, N_BITS)
        sync = m.sync_bits
        m.sync_bits = rng.integers(0, 2, len(sync))
        try:
            cap = R.make_capture(m, rng, tx_bits, MOD, R.F0, d)
        finally:
            m.sync_bits = sync
        bits, stats, calls = recorded(SM, m, cap)
        assert bits is None and stats["error"] == "Could not decode" and stats["success"] is False, stats
        assert set(stats) == {"success", "n_samples", "burst_start", "freq_offset", "sync_peak", "sync_start", "error"}
        check_front(m, stats, calls)
        bers = sync_bers(m, calls)
        assert np.min(bers) > 0.3, bers           # the check is sync_ber > 0.2: 16 bits of margin
        assert "_carrier_recovery_data" not in calls
        assert cap.dtype == np.complex64 and -(-len(cap) // TILE) == 8
        out["cap_nosync"] = cap
        for key in ("burst_start", "freq_offset", "sync_peak", "sync_start"):
            out[key + "_nosync"] = np.asarray(stats[key])
        print("nosync: burst_start", stats["burst_start"], "sync_start", stats["sync_start"], "sync BERs", bers.ravel())

        # ---- rot ------------------------------------------------------------------------------
        rng = np.random.default_rng([SEED, 1])
        tx_bits = rng.integers(0, 2, N_BITS)
        phi = R.PHI
        R.PHI = phi + np.pi
        try:
            cap = R.make_capture(m, rng, tx_bits, MOD, R.F0, d)
        finally:
            R.PHI = phi
        bits, stats, calls = recorded(SM, m, cap)
        assert stats["success"] and np.array_equal(bits, tx_bits), "the fixture must decode without errors"
        check_front(m, stats, calls)
        bers = sync_bers(m, calls)
        assert np.all(np.abs(bers - 0.2) > 0.03), bers          # five bits from the check, every decision clear
        passing = [(k, rot) for k in range(m.sps) for rot in range(2) if bers[k, rot] <= 0.2]
        assert passing and all(rot == 1 for _, rot in passing), passing
        assert len(passing) >= 2, "more than one timing offset must reach the data loop"
        cb, cd = calls["_carrier_recovery_bpsk"], calls["_carrier_recovery_data"]
        assert len(cd) == len(passing)
        for (k, rot), (a, _, _) in zip(passing, cd):          # the recorded call says so itself
            assert a[1] == cb[k][2][1] + np.pi and a[1] != cb[k][2][1] and a[2] == cb[k][2][2] and a[3] == MOD
        # the accepted candidate: the first of the lowest sync BER, at data rotation 0
        best = min(range(len(passing)), key=lambda j: (bers[passing[j]], j))
        rec = cd[best][2]
        assert np.array_equal(stats["rx_symbols"], rec / np.sqrt(np.mean(np.abs(rec) ** 2)) * np.exp(1j * 0 * np.pi / 2))
        assert stats["sync_ber"] == bers[passing[best]]
        assert R.boundary_margin(stats["rx_symbols"], MOD) > 1e-6
        assert cap.dtype == np.complex64 and -(-len(cap) // TILE) == 8
        out["cap_rot"], out["tx_bits_rot"], out["bits_rot"] = cap, tx_bits, np.asarray(bits)
        for key in ("burst_start", "freq_offset", "sync_peak", "sync_start", "sync_ber", "rx_symbols"):
            out[key + "_rot"] = np.asarray(stats[key])
        out["cr_data_par_rot"] = np.array([[a[1], a[2], a[4]] for a, _, _ in cd])
        out["sync_rot_rot"] = np.int64(passing[best][1])
        out["n_offsets_rot"] = np.int64(len({k for k, _ in passing}))
        print("rot: burst_start", stats["burst_start"], "sync_start", stats["sync_start"], "sync BERs", bers.ravel(),
              "accepted (offset, sync_rot)", passing[best])

    for k, v in out.items():
        assert v.dtype.kind in "cfiu" and v.dtype in (np.complex64, np.complex128, np.float64, np.int64), (k, v.dtype)
    path = os.path.join(R.OUT, "rx_paths.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print("wrote", path, len(out), "arrays", size, "bytes")


if __name__ == "__main__":
    main()
