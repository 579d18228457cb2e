"""The mixer and the carrier loops on the cases of tests/rx_loops.py (tests/test_rx_loops_host.py
keeps their conditions and census), and SDRModem._process_received on the two captures of
tests/golden/rx_paths.npz (make_golden_rx_paths.py).

Mixer: every case through mix / mix_device and through mdm_mix / mdm_mix_dev called directly; the
four must agree bit for bit.  Exact cases (w = 0) against the float64 restatement and, where the
angle is +0, numpy's own (sig - dc) * (1 + 0j); toleranced ones within 8 eps |sig - dc| of the
long double restatement.  Carrier loops: every case through mdm_carrier and mdm_carrier_dev, bit-equal to
each other; exact cases bit-equal to the float64 restatement, toleranced ones within 16 times the
float64 restatement's own distance from the long double one (floored at 1e-10 n / 2000)."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulations_amd import _native as NT  # noqa: E402
from modulations_amd import modem as MM  # noqa: E402

import rx_loops as X  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = X.carrier_cases()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------- mixer --------------------------
def mix_four_ways(sig, dc, w, fs, i0):
    """The output of mix, after asserting that the other three entry points give the same bits."""
    L = NT.modem_lib()
    y = MM.mix(sig, w, fs, dc=dc, i0=i0)
    d_sig = torch.from_numpy(sig).cuda()
    d = MM.mix_device(d_sig, w, fs, dc=dc, i0=i0).cpu().numpy()
    dcv = MM._dc(dc)
    f64, dcp = int(sig.dtype == np.complex128), NT.ptr(dcv)
    raw = np.full(len(sig), np.nan + 0j, np.complex128)
    NT.modem_check(L.mdm_mix(0, NT.ptr(sig), f64, len(sig), i0, dcp, w, fs, NT.ptr(raw)))
    d_raw = torch.full((len(sig),), float("nan"), dtype=torch.complex128, device="cuda")
    NT.modem_check(L.mdm_mix_dev(0, NT.ptr(d_sig), f64, len(sig), i0, dcp, w, fs, NT.ptr(d_raw),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for name, other in (("mix_device", d), ("mdm_mix", raw), ("mdm_mix_dev", d_raw.cpu().numpy())):
        assert X.same_bits(other, y), name
    return y


@pytest.mark.parametrize("k", range(len(X.mix_cases())), ids=[c.name for c in X.mix_cases()])
def test_mix_case(k):
    c = X.mix_cases()[k]
    sig, dc = X.mix_inputs(c)
    y = mix_four_ways(sig, dc, c.w, X.MIX_FS, c.i0)
    assert y.shape == (c.n,) and y.dtype == np.complex128
    if c.exact:
        assert X.same_bits(y, X._cplx(*X.mix_ref(sig, dc, c.w, X.MIX_FS, c.i0)))
        if c.i0 >= 0:
            ref = X.mix_numpy_w0(sig, dc)
            assert np.array_equal(np.isnan(y.view(np.float64)), np.isnan(ref.view(np.float64)))
            assert X.same_bits(y, ref)
    else:
        bound = X.mix_bound(sig, dc)
        err = X.mix_distance(y, X.mix_ref(sig, dc, c.w, X.MIX_FS, c.i0, X.LD))
        print(f"mix {c.name}: max |delta| / (eps |sig - dc|) = {float(np.max(err / (bound / 8))):.3g}")
        assert np.all(err <= bound)


# ---------------------------------------------------------------- carrier loops -------------------
def carrier_both_ways(c):
    """(out, final) of mdm_carrier, after asserting that mdm_carrier_dev gives the same bits."""
    out, fin = MM.carrier_recovery(c.syms, c.ph, c.fr, c.al, c.kind)
    d_out, d_fin = MM.carrier_recovery_device(torch.from_numpy(np.array(c.syms)).cuda(), c.ph, c.fr, c.al,
                                              c.kind)
    assert X.same_bits(d_out.cpu().numpy(), out) and X.same_bits(d_fin.cpu().numpy(), fin), c.name
    assert out.shape == c.syms.shape and fin.shape == (c.syms.shape[0], 2)
    return out, fin


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.exact and c.family not in ("nan", "coast")])
def test_carrier_exact(name):
    c = CASES[name]
    out, fin = carrier_both_ways(c)
    ref_out, ref_fin = X.carrier_f64(c)
    bad = [i for i in range(len(out)) if not (X.same_bits(out[i], ref_out[i]) and X.same_bits(fin[i], ref_fin[i]))]
    assert not bad, (name, bad[:8], [(int(c.kind[i]), c.syms[i, 0], out[i, 0], ref_out[i, 0], fin[i], ref_fin[i])
                                     for i in bad[:3]])
    if name == "still":
        assert X.same_bits(out, c.syms) and X.same_bits(fin, np.zeros((3, 2)))


def test_carrier_coasting_final_is_exact():
    """alpha = 0 from phase0 = 0 with a frequency: the final state is 300 additions, whatever sincos
    returns on the way; step 0 (phase 0) passes the sample through."""
    c = CASES["coast"]
    out, fin = carrier_both_ways(c)
    ref_out, ref_fin = X.carrier_f64(c)
    assert X.same_bits(fin, ref_fin) and X.same_bits(out[:, 0], c.syms[:, 0])
    d = np.max(np.abs(out - ref_out) / np.abs(c.syms), axis=1)
    print("carrier coast: max |out - float64 restatement| / |s| per stream =", d)
    assert np.all(d <= X.RTOL * 300 / X.RTOL_N)      # |phase| <= 900 rad: the sincos of a known double


def test_carrier_nan_stays_in_its_lane():
    clean, dirty = CASES["nan_clean"], CASES["nan"]
    (o0, f0), (o1, f1) = carrier_both_ways(clean), carrier_both_ways(dirty)
    hit = np.zeros(X.CR_BLOCK, bool)
    for lane, step, _ in X.NAN_AT:
        hit[lane] = True
        assert X.same_bits(o1[lane, :step], o0[lane, :step])
        assert np.isnan(o1[lane, step:].real).all() and np.isnan(o1[lane, step:].imag).all()
        assert np.isnan(f1[lane]).all()
    assert np.isfinite(o0.view(np.float64)).all() and np.isfinite(f0).all()
    assert X.same_bits(o1[~hit], o0[~hit]) and X.same_bits(f1[~hit], f0[~hit])


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.exact])
def test_carrier_toleranced(name):
    c = CASES[name]
    out, fin = carrier_both_ways(c)
    ref, cpu, bound = X.carrier_refs(name)
    gpu = X.carrier_distance(out, fin, ref, c.syms)
    print(f"carrier {name}: distance from the long double restatement, float64 restatement: out "
          f"{float(cpu[0].max()):.3g}, final {float(cpu[1].max()):.3g}; device: out {float(gpu[0].max()):.3g}, "
          f"final {float(gpu[1].max()):.3g}; worst device / bound: out {float(np.max(gpu[0] / bound[0])):.3g}, "
          f"final {float(np.max(gpu[1] / bound[1])):.3g}")
    assert np.all(gpu[0] <= bound[0]) and np.all(gpu[1] <= bound[1])


def test_carrier_dev_unknown_kind_is_nan_in_its_lane_only():
    """include/modem.h: the _dev form cannot read the kinds; an unknown one yields NaNs (the host
    form and the wrappers refuse it, so the entry point is called directly)."""
    c = CASES["batch65"]
    good_out, good_fin = carrier_both_ways(c)
    kind = c.kind.copy()
    bad = np.zeros(65, bool)
    for lane, k in ((3, 3), (40, -1), (64, 1 << 30)):
        kind[lane], bad[lane] = k, True
    dev = torch.device("cuda")
    t = [torch.from_numpy(np.array(a)).to(dev) for a in (c.syms, c.ph, c.fr, c.al, kind)]
    d_out = torch.zeros(c.syms.shape, dtype=torch.complex128, device=dev)
    d_fin = torch.zeros((65, 2), dtype=torch.float64, device=dev)
    NT.modem_check(NT.modem_lib().mdm_carrier_dev(0, NT.ptr(t[0]), 65, c.syms.shape[1], NT.ptr(t[1]), NT.ptr(t[2]),
                                                  NT.ptr(t[3]), NT.ptr(t[4]), NT.ptr(d_out), NT.ptr(d_fin),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    out, fin = d_out.cpu().numpy(), d_fin.cpu().numpy()
    assert X.same_bits(out[~bad], good_out[~bad]) and X.same_bits(fin[~bad], good_fin[~bad])
    assert np.isnan(fin[bad]).all()
    # step 0 is rotated by the given phase before any detector runs; every later output is NaN
    assert X.same_bits(out[bad, 0], good_out[bad, 0])
    assert np.isnan(out[bad, 1:].real).all() and np.isnan(out[bad, 1:].imag).all()
    ref_re, _, ref_fin = X.carrier_run(c.syms, c.ph, c.fr, c.al, kind)
    assert np.array_equal(np.isnan(ref_re), np.isnan(out.real)) and np.array_equal(np.isnan(ref_fin), np.isnan(fin))


# ---------------------------------------------------------------- _process_received ---------------
@pytest.fixture(scope="module")
def GP():
    return np.load(os.path.join(ROOT, "tests", "golden", "rx_paths.npz"), allow_pickle=False)


def test_process_received_sync_word_fails(GP):
    """A burst whose sync word is not the receiver's: no (offset, rotation) passes the sync check."""
    modem = MM.SDRModem(fs=float(GP["fs"]))
    cap = GP["cap_nosync"]
    bits, stats = modem._process_received(cap, "QPSK", int(GP["n_bits"]))
    assert bits is None
    peak = stats.pop("sync_peak")
    assert abs(peak - float(GP["sync_peak_nosync"])) <= 1e-11 * float(GP["sync_peak_nosync"])
    assert stats == {"success": False, "n_samples": len(cap), "burst_start": int(GP["burst_start_nosync"]),
                     "freq_offset": float(GP["freq_offset_nosync"]), "sync_start": int(GP["sync_start_nosync"]),
                     "error": "Could not decode"}


def test_process_received_second_sync_rotation_wins(GP):
    """The sync loop locks half a turn off: the accepted candidate starts the data loop at the
    sync loop's final phase + pi, and two timing offsets reach the data loop.  The assertions of
    test_gpu_rx.py::test_process_received_golden."""
    modem = MM.SDRModem(fs=float(GP["fs"]))
    cap, mod = GP["cap_rot"], "QPSK"
    assert int(GP["sync_rot_rot"]) == 1 and int(GP["n_offsets_rot"]) >= 2
    seen = []
    inner = MM.carrier_recovery_device

    def spy(syms, init_phase, init_freq, alpha, kind, **kw):
        out, fin = inner(syms, init_phase, init_freq, alpha, kind, **kw)
        seen.append((np.asarray(init_phase, np.float64), fin.cpu().numpy()))
        return out, fin
    MM.carrier_recovery_device = spy
    try:
        bits, stats = modem._process_received(cap, mod, int(GP["n_bits"]))
    finally:
        MM.carrier_recovery_device = inner
    assert set(stats) == {"success", "n_samples", "burst_start", "freq_offset", "sync_peak", "sync_start",
                          "sync_ber", "rx_symbols"}
    assert stats["success"] is True and stats["n_samples"] == len(cap)
    assert stats["burst_start"] == int(GP["burst_start_rot"])
    assert stats["freq_offset"] == float(GP["freq_offset_rot"])
    assert stats["sync_start"] == int(GP["sync_start_rot"])
    assert abs(stats["sync_peak"] - float(GP["sync_peak_rot"])) <= 1e-11 * float(GP["sync_peak_rot"])
    assert stats["sync_ber"] == float(GP["sync_ber_rot"])
    ref = GP["rx_symbols_rot"]
    print("rx_symbols: max relative delta =", np.max(np.abs(stats["rx_symbols"] - ref) / np.abs(ref)))
    np.testing.assert_allclose(stats["rx_symbols"], ref, rtol=1e-9, atol=0)
    assert bits.dtype == GP["bits_rot"].dtype and np.array_equal(bits, GP["bits_rot"])
    assert np.array_equal(bits, GP["tx_bits_rot"])
    # the data loop's initial phases: every candidate is some sync stream's final phase + pi
    (_, sync_fin), (data_ph, _) = seen
    par = GP["cr_data_par_rot"]
    assert len(data_ph) == len(par) >= 2
    np.testing.assert_allclose(data_ph, par[:, 0], rtol=1e-10, atol=0)
    for ph in data_ph:
        assert np.any(sync_fin[:, 0] + np.pi == ph) and not np.any(sync_fin[:, 0] == ph)
