"""Receive diversity, the parts that need no GPU: the numpy
restatement of the combiner (tests/mrc_ref.py) against the equaliser's restatement and
against itself, the ABI names, the refusals that come before any device call and the
BER sweep's option."""
import os
import re

import numpy as np
import pytest

import fading_ref as F
import mrc_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tdec_combine_dev", "tdec_workload_branches_dev", "tdec_workload_frame_branches_dev")
U = 2.0 ** -53                                          # float64 unit roundoff


def _bits_equal(a, b):
    """IEEE ==, NaN at the same positions, and the same zeros' signs."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype in (np.float32, np.complex64) else np.uint64
    na, nb = np.isnan(a.view(a.real.dtype)), np.isnan(b.view(b.real.dtype))
    return np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


def _cn(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)


def _special(rng, B, S, nh):
    """y [B, S] and h [B, nh] over many decades with the equaliser tests' special values."""
    y = (_cn(rng, B, S) * np.float32(10) ** rng.integers(-3, 4, (B, S))).astype(np.complex64)
    h = (_cn(rng, B, nh) * np.float32(10) ** rng.integers(-2, 3, (B, nh))).astype(np.complex64)
    sh = np.array([0, 1e-42 + 3e-43j, np.nan + 1j, 1 + np.inf * 1j, -np.inf, 1e25 - 1e25j, 1e-30j], np.complex64)
    sy = np.array([np.nan, np.inf + 1j, 1 - np.inf * 1j, 0, 1e38 + 1e38j, 1e-44, complex(-0.0, -0.0)], np.complex64)
    hf, yf = h.reshape(-1), y.reshape(-1)
    hi = rng.permutation(hf.size)[:len(sh)]
    hf[hi] = sh[:len(hi)]
    yi = rng.permutation(yf.size)[:len(sy)]
    yf[yi] = sy[:len(yi)]
    return y, h


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("B,S,coh", [(5, 37, 1), (3, 40, 7), (2, 16, 16)])
def test_one_branch_with_common_noise_is_the_equaliser(B, S, coh, rows):
    rng = np.random.default_rng(B * S + coh + rows)
    y, h = _special(rng, B, S, -(-S // coh))
    nv = 10.0 ** rng.uniform(-3, 1, B) if rows else 0.0371
    z, nvs = MR.combine(y[:, None], h[:, None], nv, coh)
    rz, rnv = F.equalize(y, h, nv, coh)
    assert _bits_equal(z, rz) and _bits_equal(nvs, rnv)
    assert np.isposinf(nvs).any()                                     # the zero gain's erasures are in there


def test_a_negative_zero_numerator_keeps_its_sign():
    """y = -0 - 0j through h = 1 + 1j: yr*hr + yi*hi = -0.0, and 0.0 + -0.0 would be +0.0."""
    y = np.array([[[complex(-0.0, -0.0)]]], np.complex64)
    h = np.array([[[1 + 1j]]], np.complex64)
    z, _ = MR.combine(y, h, 0.1)
    rz, _ = F.equalize(y[:, 0], h[:, 0], 0.1)
    assert np.signbit(rz.real[0, 0]) and _bits_equal(z, rz)
    # and behind a dead branch: the sum starts from the first LIVE branch's term
    y2 = np.concatenate([np.ones((1, 1, 1), np.complex64), y], axis=1)
    h2 = np.concatenate([np.zeros((1, 1, 1), np.complex64), h], axis=1)
    assert _bits_equal(MR.combine(y2, h2, 0.1)[0], rz)


def test_equal_per_branch_noise_agrees_with_the_common_form():
    """R = 2, nv_br = nv for both branches.  With u = 2^-53, Sa = |a_0| + |a_1| and Sg = g_0 + g_1:
    the per-branch form rounds each term's division by nv (the two extra roundings) before the sum.
    G' nv = Sg (1 + t), |t| <= 2u (all terms positive), G = Sg (1 + e): nv / G and 1 / G', each rounded
    once more, differ by at most 5u relative, which is under 5 ulp (ulp(x) > u |x|).  The numerators
    may cancel, so their bound is absolute: |A' nv - (a_0 + a_1)| <= 2u Sa and |A - (a_0 + a_1)| <= u Sa;
    with the denominators' and the quotients' roundings the two float64 quotients differ by at most
    (5u + 3u) Sa / Sg, 9u with the second-order terms, and the casts to float32 add one float32 ulp."""
    rng = np.random.default_rng(14)
    B, S, nv = 6, 64, 0.0371
    y = _cn(rng, B, 2, S)
    h = _cn(rng, B, 2, S)
    zc, nc = MR.combine(y, h, nv)
    zb, nb = MR.combine(y, h, np.full((B, 2), nv))
    ulp64 = np.spacing(np.maximum(nc, nb))
    worst_nv = np.max(np.abs(nc - nb) / ulp64)
    hr, hi, yr, yi = (v.astype(np.float64) for v in (h.real, h.imag, y.real, y.imag))
    sg = (hr * hr + hi * hi).sum(axis=1)
    worst_z = 0.0
    for got, ref, terms in ((zb.real, zc.real, yr * hr + yi * hi), (zb.imag, zc.imag, yi * hr - yr * hi)):
        slack = np.spacing(np.maximum(np.abs(got), np.abs(ref))).astype(np.float64) + 9 * U * np.abs(terms).sum(axis=1) / sg
        worst_z = max(worst_z, np.max(np.abs(got.astype(np.float64) - ref) / slack))
    print("nv_sym: worst", worst_nv, "ulp (bound 5);  z: worst", worst_z, "of its bound")
    assert worst_nv <= 5 and worst_z <= 1.0
    assert not _bits_equal(nc, nb)                                    # and it is indeed not bit for bit


@pytest.mark.parametrize("per_branch", [False, True])
def test_a_zero_gain_branch_leaves_the_other_branch_alone(per_branch):
    rng = np.random.default_rng(3 + per_branch)
    B, S, coh = 4, 21, 5
    nh = -(-S // coh)
    y, h = _cn(rng, B, 2, S), _cn(rng, B, 2, nh)
    nv = 10.0 ** rng.uniform(-2, 0, (B, 2)) if per_branch else 0.2
    for dead in (0, 1):
        hd = h.copy()
        hd[:, dead] = 0
        alone = MR.combine(y[:, 1 - dead:2 - dead], h[:, 1 - dead:2 - dead], nv[:, 1 - dead:2 - dead] if per_branch else nv, coh)
        both = MR.combine(y, hd, nv, coh)
        assert _bits_equal(both[0], alone[0]) and _bits_equal(both[1], alone[1])
    if not per_branch:                                                # and that single-branch result is the equaliser's
        assert _bits_equal(alone[0], F.equalize(y[:, 0], h[:, 0], nv, coh)[0])
    # both dead: an erasure
    z, nvs = MR.combine(y, np.zeros_like(h), nv, coh)
    assert not z.any() and np.isposinf(nvs).all()


def test_nan_noise_stays_nan_and_infinite_weights_erase():
    y = np.ones((3, 2, 4), np.complex64)
    h = np.ones((3, 2, 4), np.complex64)
    nv = np.array([[0.1, np.nan], [0.0, 0.1], [np.inf, np.inf]])
    z, nvs = MR.combine(y, h, nv)
    assert np.isnan(z[0].real).all() and np.isnan(nvs[0]).all()       # section 10's convention, not a skip
    for r in (1, 2):                                                  # G = inf and G = 0
        assert not z[r].any() and np.isposinf(nvs[r]).all()
    h[0, 0] = 1e30                                                    # |h|^2 overflows float32's range, not float64's
    z, nvs = MR.combine(y, h, 0.1)
    assert np.isfinite(nvs).all() and nvs[0, 0] < 1e-59


def test_branch_gains_extend_the_single_branch_draw():
    g = MR.gains(np.arange(5, 9), 3, 11, 4242, K=4.0)
    assert g.shape == (4, 3, 11)
    assert np.array_equal(g[:, 0], F.gains(np.arange(5, 9), 11, 4242, K=4.0))
    assert not np.array_equal(g[:, 1], g[:, 0]) and not np.array_equal(g[:, 2], g[:, 1])


# ---- names, refusals in front of the device, the sweep's option ------------------------------
def test_names_are_exported_and_declared():
    from modulations_amd import _native
    with open(os.path.join(ROOT, "include", "tdec.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _native.EXPORTS
        assert re.search(rf"^int {name}\(", header, re.M), name


def test_combine_device_refuses_before_any_device_call():
    torch = pytest.importorskip("torch")
    from modulations_amd import demap as D
    y = torch.zeros((2, 2, 6), dtype=torch.complex64)
    with pytest.raises(TypeError):
        D.combine_device(y.to(torch.complex128), y, 0.1)
    with pytest.raises(TypeError):
        D.combine_device(y, y.real, 0.1)
    with pytest.raises(ValueError, match="3-D"):
        D.combine_device(y[0], y[0], 0.1)
    with pytest.raises(ValueError, match="HIP device"):
        D.combine_device(y, y, 0.1)


def test_sweep_records_the_branches_only_when_there_are_several():
    pytest.importorskip("torch")
    from modulations_amd import ber
    ap = ber.arg_parser()
    base = ["--channel", "rayleigh", "--coherence", "106"]
    one, dflt = ap.parse_args(base + ["--rx-branches", "1"]), ap.parse_args(base)
    assert ber.sweep_config(one) == ber.sweep_config(dflt) and "rx_branches" not in ber.sweep_config(one)
    assert ber.channel_fading(one) == {"K": 0.0, "coh": 106}           # the call without the key: the same data
    two = ap.parse_args(base + ["--rx-branches", "2", "--csi", "pilots"])
    assert ber.sweep_config(two)["rx_branches"] == 2 and ber.channel_fading(two)["branches"] == 2
    assert "array gain" in ap.format_help()
    for bad in (["--rx-branches", "2"], base + ["--rx-branches", "9"], base + ["--rx-branches", "0"]):
        with pytest.raises(SystemExit):
            ber.main(bad)
