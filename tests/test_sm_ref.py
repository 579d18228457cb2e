"""Spatial multiplexing, the parts that need no GPU: the numpy restatement
of the joint detector (tests/sm_ref.py) against closed forms and against itself, the ABI names, the
refusals that come before any device call and the BER sweep's option."""
import os
import re

import numpy as np
import pytest

import sm_ref as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                                          # float64 unit roundoff


def _cn(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)


def _cons(mod):
    from modulations_amd import demap as D
    return D.constellation(mod), D.MODULATIONS[mod]["bps"]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _label_bits(lab, bps):
    return (lab[..., None] >> np.arange(bps - 1, -1, -1)) & 1


@pytest.mark.parametrize("mod", ["BPSK", "QPSK", "8PSK", "16QAM", "64QAM"])
@pytest.mark.parametrize("S", [12, 7])
def test_noise_free_input_recovers_the_labels(mod, S):
    """R = 2, y = h0 x[2m] + h1 x[2m+1] rounded to float32: the sent pair's D is of the order of the rounding
    (1e-14), every other hypothesis' is |H (dx)|^2 with H the 2 x 2 Gaussian matrix, so each bit's sign is the
    sent bit's (positive for bit 1 at sign = +1), the single-stream slot of the odd S included."""
    cons, bps = _cons(mod)
    rng = np.random.default_rng(S + bps)
    B, T, coh = 3, SM.slots_of(S), 2
    lab = rng.integers(0, len(cons), (B, S))
    x = cons.astype(np.complex64)[lab]
    h = _cn(rng, B, 2, 2, -(-T // coh))
    y = SM.signal32(h, x, coh)
    for sign in (+1, -1):
        llr = SM.detect(y, h, cons, 0.1, S=S, coh=coh, sign=sign)
        assert llr.shape == (B, S * bps) and llr.dtype == np.float32
        assert np.array_equal((sign * llr > 0).reshape(B, S, bps), _label_bits(lab, bps) == 1)
        assert np.all(llr != 0)


@pytest.mark.parametrize("sign", [+1, -1])
def test_a_silent_second_antenna_gives_stream_one_signed_zeros(sign):
    """h_r1 = 0: every b gives the same D, so m0 == m1, m0 - m1 = +0.0, +0.0 / nve = +0.0, and the written
    value is sign * +0.0f."""
    cons, bps = _cons("16QAM")
    rng = np.random.default_rng(4)
    B, R, T = 3, 2, 5
    y, h = _cn(rng, B, R, T), _cn(rng, B, R, 2, T)
    h[:, :, 1] = 0
    for nv in (0.2, np.full(B, 0.2), np.full((B, R), 0.2)):
        llr = SM.detect(y, h, cons, nv, sign=sign).reshape(B, T, 2, bps)
        assert not llr[:, :, 1].any() and np.all(np.signbit(llr[:, :, 1]) == (sign < 0))
        assert llr[:, :, 0].all()


@pytest.mark.parametrize("mod", ["QPSK", "8PSK", "16QAM"])
def test_one_branch_unit_gain_is_compute_llrs_formula(mod):
    """R = 1, h0 = 1, h1 = 0: u = y - (1 c.re - 0 c.im, 1 c.im + 0 c.re) = y - c exactly, v = u - 0, so stream
    0's LLRs are the single-antenna max-log formula, (min_0 |y - c|^2 - min_1 |y - c|^2) / nve clipped,
    evaluated directly in float64 with |.|^2 = re^2 + im^2."""
    cons, bps = _cons(mod)
    rng = np.random.default_rng(7)
    B, T, nv = 4, 9, 0.3
    y = _cn(rng, B, 1, T)
    h = np.zeros((B, 1, 2, 1), np.complex64)
    h[:, :, 0] = 1
    got = SM.detect(y, h, cons, nv, coh=T).reshape(B, T, 2, bps)[:, :, 0]
    yr, yi = y[:, 0].real.astype(np.float64), y[:, 0].imag.astype(np.float64)
    cr, ci = cons.real.astype(np.float64), cons.imag.astype(np.float64)
    d = np.stack([(yr - cr[a]) * (yr - cr[a]) + (yi - ci[a]) * (yi - ci[a]) for a in range(len(cons))])   # [M, B, T]
    bits = _label_bits(np.arange(len(cons)), bps)
    for j in range(bps):
        m0, m1 = d[bits[:, j] == 0].min(axis=0), d[bits[:, j] == 1].min(axis=0)
        assert _bits_equal(got[:, :, j], np.clip((m0 - m1) / nv, -30, 30).astype(np.float32))


def test_the_last_slot_of_an_odd_length_is_single_stream():
    cons, bps = _cons("8PSK")
    rng = np.random.default_rng(9)
    B, R, S = 2, 2, 7
    T = SM.slots_of(S)
    y, h = _cn(rng, B, R, T), _cn(rng, B, R, 2, T)
    llr = SM.detect(y, h, cons, 0.2, S=S)
    assert llr.shape == (B, S * bps)
    h2 = h.copy()
    h2[:, :, 1, -1] = _cn(rng, B, R)                                  # antenna 1's gain there is not read
    assert _bits_equal(SM.detect(y, h2, cons, 0.2, S=S), llr)
    alone = SM.detect(y[:, :, -1:], h[:, :, :, -1:], cons, 0.2, S=1)  # the slot by itself
    assert _bits_equal(alone, llr[:, -bps:]) and alone.all()
    even = SM.detect(y, h, cons, 0.2)                                 # S = 2 T: the same slots before it
    assert _bits_equal(even[:, :(S - 1) * bps], llr[:, :(S - 1) * bps])
    assert not _bits_equal(even[:, (S - 1) * bps:S * bps], llr[:, -bps:])


@pytest.mark.parametrize("form", ["scalar", "rows", "branches"])
def test_skip_and_erasure_rules(form):
    cons, bps = _cons("QPSK")
    rng = np.random.default_rng(11)
    B, R, T = 4, 3, 6
    y, h = _cn(rng, B, R, T), _cn(rng, B, R, 2, T)
    nv = {"scalar": 0.2, "rows": 10.0 ** rng.uniform(-2, 0, B), "branches": 10.0 ** rng.uniform(-2, 0, (B, R))}[form]
    ref = SM.detect(y, h, cons, nv)
    for dead in range(R):
        keep = [r for r in range(R) if r != dead]
        alone = SM.detect(y[:, keep], h[:, keep], cons, nv[:, keep] if form == "branches" else nv)
        for poison in ("h0", "h1", "y", "inf"):
            yd, hd = y.copy(), h.copy()
            if poison == "y":
                yd[:, dead, 2] = complex(1.0, np.nan)
            elif poison == "inf":
                hd[:, dead, 1, 2] = complex(-np.inf, 0.0)
            else:
                hd[:, dead, int(poison[1]), 2] = complex(np.nan, 0.0)
            got = SM.detect(yd, hd, cons, nv).reshape(B, T, 2 * bps)
            assert _bits_equal(got[:, 2], alone.reshape(B, T, 2 * bps)[:, 2])   # skipped in that slot only
            keep_slots = [0, 1, 3, 4, 5]
            assert _bits_equal(got[:, keep_slots], ref.reshape(B, T, 2 * bps)[:, keep_slots])
    # zero gains are live: every hypothesis gives D = sum |y_r|^2, so every LLR is sign * +0.0f -- at sign = -1
    # a negative zero, where an erasure writes +0.0f
    got = SM.detect(y, np.zeros_like(h), cons, nv, sign=-1)
    assert not got.any() and np.signbit(got).all()
    for sign in (+1, -1):                                             # no live branch: +0.0f whatever the sign
        yd = y.copy()
        yd[1, :, 3] = np.nan
        got = SM.detect(yd, h, cons, nv, sign=sign).reshape(B, T, 2 * bps)
        assert not got[1, 3].any() and not np.signbit(got[1, 3]).any()
        assert got[1, 2].all() and got[0, 3].all()


def test_noise_floor_nan_and_infinite_noise():
    cons, bps = _cons("16QAM")
    rng = np.random.default_rng(13)
    B, R, T = 3, 2, 4
    y, h = np.float32(0.03) * _cn(rng, B, R, T), np.float32(0.03) * _cn(rng, B, R, 2, T)
    at_floor = SM.detect(y, h, cons, 0.005)
    assert np.abs(at_floor).max() < 30                                # the clip does not hide the comparison
    for nv in (0.001, 0.0, -1.0, np.nan):
        assert _bits_equal(SM.detect(y, h, cons, nv), at_floor)
        assert _bits_equal(SM.detect(y, h, cons, np.full(B, nv)), at_floor)
    rows = np.array([0.3, np.nan, np.inf])
    got = SM.detect(y, h, cons, rows)
    assert _bits_equal(got[0:1], SM.detect(y[0:1], h[0:1], cons, 0.3))
    assert _bits_equal(got[1:2], at_floor[1:2])
    assert not got[2].any()                                           # +inf: zero LLRs
    br = np.full((B, R), 0.3)
    br[1, 0], br[2, :] = np.nan, np.inf
    want = br.copy()
    want[1, 0] = 0.005
    got = SM.detect(y, h, cons, br)
    assert _bits_equal(got[:2], SM.detect(y[:2], h[:2], cons, want[:2])) and not got[2].any()
    br[2, 1] = 0.3                                                    # one infinite branch: its term is 0, the other decides
    assert _bits_equal(SM.detect(y, h, cons, br)[2:], SM.detect(y[2:, 1:], h[2:, 1:], cons, br[2:, 1:]))


@pytest.mark.parametrize("R", [1, 2, 5])
def test_equal_per_branch_noise_agrees_with_the_common_form(R):
    """nv_br = nv for every branch.  A branch's d_r is the same float64 number in both forms.  With u = 2^-53,
    to first order: the per-branch form's D' = sum round(d_r / nve) carries one rounding per quotient and R - 1
    per sum of positive terms, D' = (sum d_r / nve)(1 + t'), |t'| <= R u; the common form's D = (sum d_r)(1 + t),
    |t| <= (R - 1) u.  So D' = (D / nve)(1 + e), |e| <= (2R - 1) u for every hypothesis, and a minimum over the
    same set keeps that bound: |m' - m / nve| <= (2R - 1) u m / nve.  LLR' = round(m0' - m1') and
    LLR = round(round(m0 - m1) / nve) add 3 roundings of values no larger than (m0 + m1) / nve, so
    |LLR' - LLR| <= (2R + 2) u (m0 + m1) / nve, (2R + 4) u with the second-order terms.  The clip is
    1-Lipschitz and the cast to float32 moves each value by at most half an ulp: one float32 ulp in all."""
    cons, bps = _cons("16QAM")
    rng = np.random.default_rng(14 + R)
    B, T, nv = 5, 8, 0.371
    y, h = _cn(rng, B, R, T), np.float32(0.5) * _cn(rng, B, R, 2, T)
    lc, m = SM.detect(y, h, cons, nv, minima=True)
    lb = SM.detect(y, h, cons, np.full((B, R), nv))
    tot = np.stack([m[2 * s, j] + m[2 * s + 1, j] for s in (0, 1) for j in range(bps)], axis=-1).reshape(B, -1)
    slack = np.spacing(np.maximum(np.abs(lc), np.abs(lb))).astype(np.float64) + (2 * R + 4) * U * tot / nv
    worst = float(np.max(np.abs(lc.astype(np.float64) - lb) / slack))
    print(f"R = {R}: worst |LLR' - LLR| over its bound {worst:.3f}")
    assert worst <= 1.0 and (np.abs(lc) < 30).mean() > 0.5            # most values are not at the clip


def test_transmit_mapping_and_signal():
    x = np.array([[1 + 2j, 3 - 4j, -5 + 6j]], np.complex64)
    a0, a1 = SM.transmit(x)
    assert np.array_equal(a0, np.array([[1 + 2j, -5 + 6j]], np.complex64))
    assert np.array_equal(a1, np.array([[3 - 4j, 0]], np.complex64))
    h = np.array([[[[2, 1j]], [[1, 1]]]], np.complex64).reshape(1, 1, 2, 2)   # antenna 0: (2, 1j), antenna 1: (1, 1)
    y = SM.signal32(h, x, 1)
    assert np.array_equal(y, np.array([[[2 * (1 + 2j) + (3 - 4j), 1j * (-5 + 6j)]]], np.complex64))


# ---- names, refusals in front of the device, the sweep's option ------------------------------
def test_names_are_exported_and_declared():
    from modulations_amd import _native, build
    with open(os.path.join(ROOT, "include", "sm.h")) as f:
        header = f.read()
    declared = re.findall(r"^int (\w+)\(", header, re.M)
    assert sorted(declared) == sorted(_native.SM_EXPORTS) == ["sm_detect_dev", "sm_workload_dev"]
    assert not set(_native.SM_EXPORTS) & (set(_native.EXPORTS) | set(_native.STBC_EXPORTS))
    assert os.path.join(ROOT, "include", "sm.h") in build.DEPS


def test_sweep_records_the_mode_only_when_it_multiplexes():
    pytest.importorskip("torch")
    from modulations_amd import ber
    ap = ber.arg_parser()
    base = ["--channel", "rayleigh", "--coherence", "106", "--mod", "QPSK"]
    stbc, dflt = ap.parse_args(base + ["--tx-antennas", "2", "--tx-mode", "stbc"]), ap.parse_args(base + ["--tx-antennas", "2"])
    assert ber.sweep_config(stbc) == ber.sweep_config(dflt) and "tx_mode" not in ber.sweep_config(dflt)
    assert ber.channel_fading(dflt)["tx_antennas"] == 2
    sm = ap.parse_args(["--channel", "rayleigh", "--coherence", "53", "--mod", "QPSK", "--tx-antennas", "2", "--tx-mode", "sm",
                        "--rx-branches", "2", "--llr", "int8", "--early-stop"])
    cfg = ber.sweep_config(sm)
    assert cfg["tx_mode"] == "sm" and cfg["tx_antennas"] == 2 and cfg["rx_branches"] == 2 and cfg["llr"] == "int8"
    assert ber.channel_fading(sm) == {"K": 0.0, "coh": 53, "branches": 2} and ber.sm_mode(sm) and not ber.sm_mode(dflt)
    assert "doubled rate is not charged" in " ".join(ap.format_help().split())
    two = base + ["--tx-antennas", "2", "--tx-mode", "sm"]
    for bad in (base + ["--tx-mode", "sm"], two + ["--csi", "pilots"], two + ["--crc", "crc16"], two + ["--harq", "chase"],
                two + ["--demap", "log-map"], two[:4] + ["--mod", "256QAM"] + two[6:],
                ["--mod", "QPSK", "--tx-antennas", "2", "--tx-mode", "sm"]):
        with pytest.raises(SystemExit):
            ber.main(bad)


def test_make_symbols_refuses_before_any_device_call():
    pytest.importorskip("torch")
    from modulations_amd import demap as D
    from modulations_amd import workload as W
    f = {"K": 0.0, "coh": 3}
    for fading, kw in ((None, {}), (f, {"pilots": D.PilotLayout(2, 8)}), (f, {"tx": 1}), (f, {"crc": "crc16"}),
                       ({**f, "coh": 4, "tx_antennas": 2}, {})):
        with pytest.raises(ValueError, match="spatial multiplexing"):
            W.make_symbols(None, 4, "QPSK", 3.0, 1, "cpu", fading=fading, streams=2, **kw)
    with pytest.raises(ValueError, match="64-point"):
        W.make_symbols(None, 4, "256QAM", 3.0, 1, "cpu", fading=f, streams=2)
    for streams in (0, 3, True, "2"):
        with pytest.raises(ValueError, match="streams"):
            W.make_symbols(None, 4, "QPSK", 3.0, 1, "cpu", fading=f, streams=streams)


def test_pipeline_refuses_before_any_device_call():
    pytest.importorskip("torch")
    from modulations_amd import workload as W
    for kw in ({"fused": True}, {"overlap": True}, {"demap": "log-map"}):
        with pytest.raises(ValueError, match="sm=True"):
            W.DevicePipeline(None, "QPSK", 4, "cpu", sm=True, **kw)
    with pytest.raises(ValueError, match="64-point"):
        W.DevicePipeline(None, "256QAM", 4, "cpu", sm=True)


def test_detect_device_refuses_before_any_device_call():
    torch = pytest.importorskip("torch")
    from modulations_amd import demap as D
    y, h = torch.zeros((2, 2, 3), dtype=torch.complex64), torch.zeros((2, 2, 2, 3), dtype=torch.complex64)
    with pytest.raises(ValueError, match="64-point"):
        D.sm_detect_device(y, h, "256QAM", 0.1)
    with pytest.raises(TypeError):
        D.sm_detect_device(y.to(torch.complex128), h, "QPSK", 0.1)
    with pytest.raises(ValueError, match="3-D"):
        D.sm_detect_device(y[0], h[0], "QPSK", 0.1)
    with pytest.raises(ValueError, match="HIP device"):
        D.sm_detect_device(y, h, "QPSK", 0.1)
