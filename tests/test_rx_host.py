"""Burst-receive chain, CPU side: argument checks of the wrappers (made before
the library is touched), build_frame's length and layout, and the C ABI list
of the new entry points."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from modulations_amd import _native
from modulations_amd import modem as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX_SYMBOLS = ("mdm_mix_dev", "mdm_mix", "mdm_burst_find_dev", "mdm_burst_find", "mdm_xcorr_peak_dev",
              "mdm_xcorr_peak", "mdm_carrier_dev", "mdm_carrier")


@pytest.fixture
def no_library(monkeypatch):
    """Any use of libmodem.so fails the test."""
    def boom():
        raise AssertionError("the wrapper touched the library before checking its arguments")
    monkeypatch.setattr(_native, "modem_lib", boom)


def test_xcorr_rejects_too_many_taps(no_library):
    with pytest.raises(ValueError):
        MM.xcorr_peak(np.zeros(4096, np.complex128), np.ones(1025, np.complex128))
    with pytest.raises(ValueError):
        MM.xcorr_peak(np.zeros(4096, np.complex128), np.ones(0, np.complex128))


def test_xcorr_rejects_short_region(no_library):
    with pytest.raises(ValueError):
        MM.xcorr_peak(np.zeros(639, np.complex128), np.ones(640, np.complex128))


def test_carrier_rejects_unknown_kind(no_library):
    s = np.ones((2, 8), np.complex128)
    with pytest.raises(ValueError):
        MM.carrier_recovery(s, 0.0, 0.0, 0.03, 3)
    with pytest.raises(ValueError):
        MM.carrier_recovery(s, 0.0, 0.0, 0.03, [MM.CR_BPSK, -1])


def test_carrier_rejects_mismatched_batch(no_library):
    s = np.ones((4, 8), np.complex128)
    with pytest.raises(ValueError):
        MM.carrier_recovery(s, np.zeros(3), 0.0, 0.03, MM.CR_BPSK)
    with pytest.raises(ValueError):
        MM.carrier_recovery(s, 0.0, 0.0, np.full(5, 0.03), MM.CR_BPSK)
    with pytest.raises(ValueError):
        MM.carrier_recovery(s, 0.0, 0.0, 0.03, [0, 1, 2])
    with pytest.raises(ValueError):
        MM.carrier_recovery(np.ones(8, np.complex128), 0.0, 0.0, 0.03, MM.CR_BPSK)   # not [C, n]


def test_burst_find_rejects_bad_window(no_library):
    x = np.zeros(2000, np.complex64)
    for win in (0, 1025):
        with pytest.raises(ValueError):
            MM.burst_find(x, 100, win=win)
    with pytest.raises(ValueError):
        MM.burst_find(x[:999], 100, win=1000)
    with pytest.raises(ValueError):
        MM.burst_find(x, -1)


def test_carrier_params_broadcast():
    ph, fr, al, kd = MM._carrier_params(3, 0.5, [0.0, 0.1, 0.2], 0.03, MM.CR_PSK8)
    assert ph.tolist() == [0.5] * 3 and fr.tolist() == [0.0, 0.1, 0.2] and al.tolist() == [0.03] * 3
    assert kd.dtype == np.int32 and kd.tolist() == [2, 2, 2]


@pytest.fixture
def host_kernels(monkeypatch):
    """build_frame's layout without a GPU: the mapper and the FIR are replaced by the C oracle."""
    monkeypatch.setattr(MM, "map_bits", lambda bits, bps, table, device=0: O.modem_map(MM._bits_u8(bits), bps, table))
    monkeypatch.setattr(MM, "fir", lambda x, taps, up=1, down=1, offset=0, n_out=None, device=0:
                        O.modem_fir(MM._syms_c(x), taps, up, down, offset, n_out))


@pytest.mark.parametrize("mod,n_bits,n_sync", [("QPSK", 240, 160), ("8PSK", 100, 160), ("64QAM", 60, 240)])
def test_build_frame_layout(host_kernels, mod, n_bits, n_sync):
    fs, sps = 200e3, 4
    m = MM.SDRModem(fs=fs, sps=sps)
    bits = np.random.default_rng(3).integers(0, 2, n_bits)
    bps = m.MODULATIONS[mod]["bps"]
    pre, pad = int(0.01 * fs), int(0.02 * fs)
    n_wave = (n_sync + -(-n_bits // bps)) * sps
    one = m.build_frame(bits, mod, n_repeats=1)
    assert one.dtype == np.complex128 and len(one) == 2 * pad + pre + n_wave
    assert not one[:pad].any() and not one[-pad:].any()
    assert np.array_equal(one[pad:pad + pre], np.ones(pre))
    wave = one[pad + pre:pad + pre + n_wave]
    sync_bits = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0] * (n_sync // 16))
    syms = np.concatenate([m._bpsk_mod(sync_bits), m.modulate(bits, mod)])
    assert np.array_equal(wave, m._upsample_filter(syms))
    # the symbol instants carry the symbols up to inter-symbol interference of the RRC pulse
    assert np.all(np.sign(wave[::sps][8:n_sync - 8].real) == np.sign(syms[8:n_sync - 8].real))
    three = m.build_frame(bits, mod, n_repeats=3)
    assert np.array_equal(three, np.tile(one, 3))
    assert len(m.build_frame(bits, mod)) == 20 * len(one)


def test_header_declares_every_rx_entry_point():
    src = open(os.path.join(ROOT, "include", "modem.h")).read()
    declared = set(re.findall(r"^\s*(?:[\w\s\*]+?)\b(mdm_\w+)\s*\(", src, re.M))
    assert set(RX_SYMBOLS) <= declared
    assert set(RX_SYMBOLS) <= set(_native.MODEM_EXPORTS)
    assert sorted(declared) == sorted(_native.MODEM_EXPORTS)
    for name in ("MDM_CR_BPSK = 0", "MDM_CR_QUAD = 1", "MDM_CR_PSK8 = 2"):
        assert name in src
    assert (MM.CR_BPSK, MM.CR_QUAD, MM.CR_PSK8) == (0, 1, 2)


def test_rx_entry_points_are_exported_and_declared():
    lib = _native.modem_lib()
    for name in RX_SYMBOLS:
        f = getattr(lib, name)
        assert f.argtypes is not None and f.restype is _native.C.c_int


def test_sdrmodem_has_the_receive_methods():
    for name in ("_estimate_freq_offset", "_correct_freq", "_carrier_recovery_bpsk", "_carrier_recovery_data",
                 "build_frame", "_process_received"):
        assert callable(getattr(MM.SDRModem, name))


def test_estimate_freq_offset_finds_a_tone():
    m = MM.SDRModem(fs=200e3)
    t = np.arange(2000) / m.fs
    assert m._estimate_freq_offset(np.exp(2j * np.pi * 5300.0 * t)) == pytest.approx(5300.0, abs=50.0)
    assert m._estimate_freq_offset(np.exp(-2j * np.pi * 7000.0 * t)) == pytest.approx(-7000.0, abs=50.0)
