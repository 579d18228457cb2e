"""The burst detector, the sync correlator and the receive chain's small entry
points at the shapes the golden captures of tests/test_gpu_rx.py never reach
(tests/golden/rx.npz: three captures of 8 tiles, silence | burst | silence).

Burst search: designed flag patterns (tests/rx_patterns.py, one per path of
k_bf_flags / k_bf_scan; tests/test_rx_patterns_host.py keeps the census) and
seeded random ones, as captures whose device flags are exactly the designed
ones; the answer is the reference's, exactly.  Smoothing: against a long double
restatement of np.convolve, within the bound include/modem.h documents.
Correlator: against a direct sum in long double, within a bound derived below,
with planted peaks for the argmax and for k_xcorr_final's strided pass.  End to
end: BPSK and 64QAM captures of the reference (tests/golden/rx_more.npz)."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulations_amd import modem as MM  # noqa: E402

import rx_patterns as RP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
LD = np.longdouble
DTYPES = (np.complex64, np.complex128)
DESIGNED = RP.designed()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def cnormal(rng, n, dtype=np.complex128):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype)


# ---------------------------------------------------------------- burst search -------------------
def pattern_signal(flags, dtype):
    """The capture of a flag pattern.  Without any set flag it is all zero (power 0, max 0,
    threshold 0: no device flag is set); amplitudes 0.5 alone would all exceed 0.3 of their own
    maximum, which is the all-set pattern."""
    if not flags.any():
        return np.zeros(len(flags), dtype), 0.0
    return RP.flags_to_signal(flags, dtype), 1.0


def check_pattern(flags, pre, device_dtype):
    want = RP.first_run(flags, pre)
    for dt in DTYPES:
        x, top = pattern_signal(flags, dt)
        start, mx, smooth = MM.burst_find(x, pre, 1, want_smooth=True)
        assert start == want, (dt.__name__, start, want)
        assert mx == top
        assert np.array_equal(smooth, (np.abs(x) ** 2).astype(np.float64))      # win = 1: exactly the power
        if dt == device_dtype:
            r = MM.burst_find_device(torch.from_numpy(x).cuda(), pre, 1)
            assert MM.burst_result(r) == (start, mx)


@pytest.mark.parametrize("k", range(len(DESIGNED)), ids=[p.name for p in DESIGNED])
def test_burst_find_designed(k):
    p = DESIGNED[k]
    check_pattern(p.flags, p.pre, DTYPES[k % 2])


RANDOM_NS = (1025, 3000, 4097, 8192, 524288 + 1031)
RANDOM_PRES = (2, 3, 10, 64, 65, 700, 2049)


@pytest.mark.parametrize("j", range(len(RANDOM_NS)), ids=[f"n{n}" for n in RANDOM_NS])
def test_burst_find_random(j):
    """300 seeded patterns in all: pattern k has n = RANDOM_NS[k % 5], pre = RANDOM_PRES[k % 7]."""
    answers = set()
    for k in range(j, 300, len(RANDOM_NS)):
        n, pre = RANDOM_NS[k % len(RANDOM_NS)], RANDOM_PRES[k % len(RANDOM_PRES)]
        flags = RP.random_flags(np.random.default_rng([20261021, k]), n, pre // 2)
        assert len(flags) == n
        check_pattern(flags, pre, DTYPES[(k // len(RANDOM_NS)) % 2])
        answers.add(RP.first_run(flags, pre))
    print(f"n = {RANDOM_NS[j]}: {len(answers)} different answers over 60 patterns")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_burst_find_dc_removed_exactly(dtype):
    """Signal + (0.25 + 0.5j) with dc = 0.25 + 0.5j: the subtraction is exact in both dtypes."""
    flags = RP.decoys(8192, 64)
    dc = 0.25 + 0.5j
    x = RP.flags_to_signal(flags, dtype)
    y = (x + dtype(dc)).astype(dtype)
    assert np.array_equal(y - dtype(dc), x)
    start, mx, smooth = MM.burst_find(y, 64, 1, dc=dc, want_smooth=True)
    assert (start, mx) == (RP.first_run(flags, 64), 1.0)
    assert np.array_equal(smooth, (np.abs(x) ** 2).astype(np.float64))
    r = MM.burst_find_device(torch.from_numpy(y).cuda(), 64, 1, dc=dc)
    assert MM.burst_result(r) == (start, mx)


# ---------------------------------------------------------------- smoothing -----------------------
SMOOTH_WINS = (1, 2, 37, 999, 1000, 1024)
SMOOTH_NS = ("win", 1024, 1025, 4096, 4097)


def smooth_ratio(x, win, dc):
    """max |device - reference| over the bound of include/modem.h, 32 eps (1024 + win) / win max(p)."""
    p = np.abs(x if dc is None else x - dc) ** 2          # in the signal's precision
    assert p.dtype == (np.float32 if x.dtype == np.complex64 else np.float64)
    ref = RP.smooth_ref(p, win)
    _, mx, smooth = MM.burst_find(x, 0, win, dc=dc, want_smooth=True)
    assert smooth.shape == ref.shape and smooth.dtype == np.float64
    assert mx == np.max(smooth)
    bound = 32 * EPS * (1024 + win) / win * float(np.max(p))
    err = float(np.max(np.abs(smooth.astype(LD) - ref)))
    assert err <= bound, (win, len(x), x.dtype, err, bound)
    return err / bound if bound else 0.0       # (one sample less its own mean: all zero)


@pytest.mark.parametrize("win", SMOOTH_WINS)
def test_smooth_bound(win):
    worst = 0.0
    for n in SMOOTH_NS:
        n = win if n == "win" else n
        if n < win:
            continue
        for dt in DTYPES:
            rng = np.random.default_rng([win, n, dt().itemsize])
            x = cnormal(rng, n, dt)
            ratio = max(smooth_ratio(x, win, np.mean(x)), smooth_ratio(x, win, None))
            assert ratio <= 1.0, (win, n, dt.__name__, ratio)
            worst = max(worst, ratio)
    print(f"smooth: win = {win}: worst |delta| / bound = {worst:.3g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_smooth_bound_one_loud_sample(dtype):
    """One sample of amplitude 1e3 among unit noise: every prefix sum behind it carries its
    rounding, and the outputs that do not cover it must still meet the bound."""
    for win in SMOOTH_WINS:
        x = cnormal(np.random.default_rng([7, win]), 4097, dtype)
        x[2500] = 1e3
        ratio = smooth_ratio(x, win, None)
        print(f"smooth, loud sample: win = {win}: |delta| / bound = {ratio:.3g}")
        assert ratio <= 1.0, (win, ratio)


# ---------------------------------------------------------------- sync search ---------------------
# Reference: ref[i] = | sum_k region[i + k] conj(w[k]) | in long double.  Bound per output:
# (2 n_w + 2) eps S[i], S[i] = sum_k |region[i + k]| |w[k]|.  Each component is a chain of 2 n_w
# fused multiply-adds, one rounding (u = eps / 2) each, over terms whose absolute sum is <= S
# (|xr wr| + |xi wi| <= |x| |w|): <= 2 n_w u S = n_w eps S per component, sqrt(2) n_w eps S for
# the complex value; the device's |z| adds <= 2 eps S.
XC_SHAPES = ((1, 1), (1, 1025), (2, 1024), (3, 2048), (5, 1023), (6, 1025), (7, 2049), (1023, 1), (1023, 1026),
             (1024, 1), (1024, 1024), (1024, 2050))
XC_PLANTS = [(n_w, n_out, i) for n_w, n_out in XC_SHAPES if n_out > 1
             for i in sorted({0, n_out - 1, 1023, 1024}) if i < n_out]
XC_STRIDE = (8, 257 * 1024 + 5)      # 258 partials: thread 0 of k_xcorr_final takes blocks 0 and 256


def xc_ref(region, w):
    n_out = len(region) - len(w) + 1
    r, h = region.astype(np.clongdouble), np.conj(w.astype(np.clongdouble))
    ar, ah = np.abs(r), np.abs(h)
    acc, S = np.zeros(n_out, np.clongdouble), np.zeros(n_out, LD)
    for k in range(len(w)):
        acc += r[k:k + n_out] * h[k]
        S += ar[k:k + n_out] * ah[k]
    return np.abs(acc), S


@functools.lru_cache(maxsize=None)
def xc_case(n_w, n_out):
    """Seeded region and taps with their reference, shared by the tests (treated as read-only)."""
    rng = np.random.default_rng([n_w, n_out])
    region, w = cnormal(rng, n_out + n_w - 1), cnormal(rng, n_w)
    ref, S = xc_ref(region, w)
    for a in (region, w, ref, S):
        a.setflags(write=False)
    return region, w, ref, S


def xc_check(region, w, ref, S, what):
    idx, peak, corr = MM.xcorr_peak(region, w, want_corr=True)
    bound = (2 * len(w) + 2) * EPS * S
    assert corr.shape == ref.shape and np.all(bound > 0)
    ratio = float(np.max(np.abs(corr.astype(LD) - ref) / bound))
    print(f"xcorr {what}: worst |delta| / bound = {ratio:.3g}")
    assert ratio <= 1.0
    assert idx == int(np.argmax(corr)) and peak == corr[idx]
    assert MM.xcorr_peak(region, w)[:2] == (idx, peak)
    return idx, peak, corr


@pytest.mark.parametrize("n_w,n_out", XC_SHAPES)
def test_xcorr_bound(n_w, n_out):
    xc_check(*xc_case(n_w, n_out), f"n_w = {n_w}, n_out = {n_out}")


def planted(n_w, n_out, at):
    """The case's region with A w added at `at`, A = 8 max|region| / rms(w), and its reference."""
    region, w, _, _ = xc_case(n_w, n_out)
    A = 8 * np.max(np.abs(region)) / np.sqrt(np.mean(np.abs(w) ** 2))
    region = region.copy()
    region[at:at + n_w] += A * w
    return (region, w) + xc_ref(region, w)


def check_planted(n_w, n_out, at):
    region, w, ref, S = planted(n_w, n_out, at)
    bound = (2 * n_w + 2) * EPS * S
    order = np.argsort(ref)
    assert order[-1] == at
    assert ref[at] - ref[order[-2]] > 2 * np.max(bound), "the planted peak must clear the runner-up by the bound"
    idx, peak, corr = xc_check(region, w, ref, S, f"n_w = {n_w}, n_out = {n_out}, peak at {at}")
    assert idx == at and corr[at] == peak


@pytest.mark.parametrize("n_w,n_out,at", XC_PLANTS)
def test_xcorr_planted_peak(n_w, n_out, at):
    check_planted(n_w, n_out, at)


@pytest.mark.parametrize("block", [256, 0])
def test_xcorr_final_second_stride_peak(block):
    """258 per-block partials: k_xcorr_final's threads 0 and 1 take two each (p += BLOCK)."""
    check_planted(*XC_STRIDE, block * 1024 + 3)


@pytest.mark.parametrize("lo,hi", [(3, 259), (0, 256)])
def test_xcorr_final_second_stride_tie(lo, hi):
    """Exactly equal maxima in two blocks that the same thread of k_xcorr_final takes, in its
    first and its second stride: the lower index wins.  Values are exact small integers, so
    np.correlate in complex128 is the reference."""
    n = 260 * 1024 + 5
    region = np.zeros(n, np.complex128)
    region[[lo * 1024 + 517, hi * 1024 + 517]] = 1.0
    w = np.ones(1, np.complex128)
    ref = np.abs(np.correlate(region, w, "valid"))
    assert len(ref) == n and np.argmax(ref) == lo * 1024 + 517 and ref[hi * 1024 + 517] == ref[lo * 1024 + 517]
    idx, peak, corr = MM.xcorr_peak(region, w, want_corr=True)
    assert (idx, peak) == (lo * 1024 + 517, 1.0) and np.array_equal(corr, ref)
    # the later one wins only when it is larger
    region[hi * 1024 + 517] = 2.0
    assert MM.xcorr_peak(region, w)[:2] == (hi * 1024 + 517, 2.0)


@pytest.mark.parametrize("n_w,n_out", [(6, 1025), (1024, 2050)])
def test_xcorr_device_form(n_w, n_out):
    region, w, _, _ = xc_case(n_w, n_out)
    idx, peak, corr = MM.xcorr_peak(region, w, want_corr=True)
    d_corr = torch.empty(n_out, dtype=torch.float64, device="cuda")
    r = MM.xcorr_peak_device(torch.from_numpy(region.copy()).cuda(), torch.from_numpy(w.copy()).cuda(), corr=d_corr)
    assert MM.xcorr_result(r) == (idx, peak)
    assert np.array_equal(d_corr.cpu().numpy(), corr)


# ---------------------------------------------------------------- mixer, carrier loops ------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_mix_in_pieces_is_the_single_call(dtype):
    cap = cnormal(np.random.default_rng(11), 5000, dtype)
    dc = np.mean(cap) if dtype == np.complex64 else None
    w, fs = (-1j * 2 * np.pi * 5300.0).imag, 200e3
    whole = MM.mix(cap, w, fs, dc=dc)
    cuts = (0, 1, 1024, 4097, 5000)
    parts = [MM.mix(cap[a:b], w, fs, dc=dc, i0=a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [len(p) for p in parts] == [1, 1023, 3073, 903]
    assert np.array_equal(np.concatenate(parts), whole)
    assert np.array_equal(whole.view(np.float64), np.concatenate(parts).view(np.float64))


@pytest.mark.parametrize("C", [1, 3])
def test_carrier_recovery_without_symbols(C):
    """n = 0: the reference's loops return an empty output and the initial phase and frequency."""
    ph, fr = np.linspace(0.3, 0.5, C), np.linspace(-0.01, 0.01, C)
    out, fin = MM.carrier_recovery(np.zeros((C, 0), np.complex128), ph, fr, 0.02, MM.CR_QUAD)
    assert out.shape == (C, 0) and out.dtype == np.complex128
    assert np.array_equal(fin, np.stack([ph, fr], axis=1))
    d_out, d_fin = MM.carrier_recovery_device(torch.zeros((C, 0), dtype=torch.complex128, device="cuda"), ph, fr,
                                              0.02, MM.CR_QUAD)
    assert tuple(d_out.shape) == (C, 0) and np.array_equal(d_fin.cpu().numpy(), fin)


@pytest.mark.parametrize("C", [1, 3])
def test_carrier_recovery_one_symbol(C):
    """n = 1: one step of sdr_modem.py:310-323 (QPSK detector), in numpy.  rtol 1e-10 as in
    tests/test_gpu_rx.py (one sin/cos of the device against numpy's, a few eps)."""
    rng = np.random.default_rng(C)
    x = cnormal(rng, C).reshape(C, 1)
    ph, fr, alpha = np.linspace(0.3, 0.5, C), np.linspace(-0.01, 0.01, C), 0.02
    out, fin = MM.carrier_recovery(x, ph, fr, alpha, MM.CR_QUAD)
    ref = x[:, 0] * np.exp(-1j * ph)
    err = np.sign(ref.real) * ref.imag - np.sign(ref.imag) * ref.real
    freq = fr + alpha * 0.1 * err
    assert out.shape == (C, 1) and fin.shape == (C, 2)
    np.testing.assert_allclose(out[:, 0], ref, rtol=1e-10, atol=0)
    np.testing.assert_allclose(fin, np.stack([ph + (alpha * err + freq), freq], axis=1), rtol=1e-10, atol=0)


# ---------------------------------------------------------------- end to end ----------------------
@pytest.fixture(scope="module")
def GM():
    return np.load(os.path.join(ROOT, "tests", "golden", "rx_more.npz"), allow_pickle=False)


@pytest.mark.parametrize("mod", ["BPSK", "64QAM"])
def test_process_received_more_modulations(GM, mod):
    """The BPSK detector of the data loop; the 240-symbol sync word (960 taps) and the QPSK-style
    detector on 64QAM.  The assertions of test_gpu_rx.py::test_process_received_golden."""
    modem = MM.SDRModem(fs=float(GM["fs"]))
    cap = GM[f"cap_{mod}"]
    bits, stats = modem._process_received(cap, mod, len(GM[f"tx_bits_{mod}"]))
    assert set(stats) == {"success", "n_samples", "burst_start", "freq_offset", "sync_peak", "sync_start",
                          "sync_ber", "rx_symbols"}
    assert stats["success"] is True and stats["n_samples"] == len(cap)
    assert stats["burst_start"] == int(GM[f"burst_start_{mod}"])
    assert stats["freq_offset"] == float(GM[f"freq_offset_{mod}"])
    assert stats["sync_start"] == int(GM[f"sync_start_{mod}"])
    assert abs(stats["sync_peak"] - float(GM[f"sync_peak_{mod}"])) <= 1e-11 * float(GM[f"sync_peak_{mod}"])
    assert stats["sync_ber"] == float(GM[f"sync_ber_{mod}"])
    ref = GM[f"rx_symbols_{mod}"]
    print("rx_symbols: max relative delta =", np.max(np.abs(stats["rx_symbols"] - ref) / np.abs(ref)))
    np.testing.assert_allclose(stats["rx_symbols"], ref, rtol=1e-9, atol=0)
    assert bits.dtype == GM[f"bits_{mod}"].dtype and np.array_equal(bits, GM[f"bits_{mod}"])
    assert np.array_equal(bits, GM[f"tx_bits_{mod}"])
    assert modem._detector(mod) == (MM.CR_BPSK if mod == "BPSK" else MM.CR_QUAD)
    assert len(modem._sync_bits_for(mod)) == (160 if mod == "BPSK" else 240)
