"""Transmit diversity, the parts that need no GPU: the numpy restatement of
the Alamouti combiner (tests/stbc_ref.py) against the equaliser's and the maximal-ratio combiner's
restatements and against itself, the ABI names, the refusals that come before any device call and
the BER sweep's option."""
import os
import re

import numpy as np
import pytest

import fading_ref as F
import mrc_ref as MR
import stbc_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                                          # float64 unit roundoff


def _cn(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)


def _bits_equal(a, b):
    """IEEE ==, NaN at the same positions, and the same zeros' signs."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype in (np.float32, np.complex64) else np.uint64
    na, nb = np.isnan(a.view(a.real.dtype)), np.isnan(b.view(b.real.dtype))
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("B,R,S,coh", [(5, 1, 37, 2), (3, 1, 40, 14), (2, 1, 16, 16), (4, 3, 21, 6)])
def test_a_silent_second_antenna_leaves_the_equaliser_on_the_even_slots(B, R, S, coh, rows):
    """h1 = 0: g = |h0|^2 + 0, the even symbol's terms are the equaliser's plus (0 + 0), and pair m uses gain
    block 2m // coh = m // (coh / 2).  IEEE == (a -0.0 numerator may come out +0.0 behind the + 0.0)."""
    rng = np.random.default_rng(B * S + coh + rows)
    S2 = SR.s2_of(S)
    nh = -(-S2 // coh)
    y = (_cn(rng, B, R, S2) * np.float32(10) ** rng.integers(-3, 4, (B, R, S2))).astype(np.complex64)
    h = np.zeros((B, R, 2, nh), np.complex64)
    h[:, :, 0] = _cn(rng, B, R, nh) * np.float32(10) ** rng.integers(-2, 3, (B, R, nh))
    h[0, :, 0, 0] = 0                                                 # an erasure
    h[1, 0, 0, -1] = 1e-42 + 3e-43j                                   # a denormal gain
    nv = 10.0 ** rng.uniform(-3, 1, B) if rows else 0.0371
    z, nvs = SR.combine(y, h, nv, S, coh)
    assert z.shape == (B, S) and nvs.shape == (B, S)
    if R == 1:
        rz, rnv = F.equalize(y[:, 0, 0::2], h[:, 0, 0], nv, coh // 2)
    else:
        rz, rnv = MR.combine(y[:, :, 0::2], h[:, :, 0], nv, coh // 2)
    assert np.array_equal(z[:, 0::2], rz) and np.array_equal(nvs[:, 0::2], rnv)
    assert np.isposinf(nvs[0, 0])


def test_noise_free_input_returns_the_points():
    """R = 1, y = h0 s0 + h1 s1 without noise.  Gains and points are random multiples of 2^-10 below 1 in
    magnitude, so the products (20 bits) and their sums are exact in float32: y holds the noise-free slots
    exactly.  In exact arithmetic num0 = G x[2m] and num1 = G x[2m+1].  The restatement's error: each part of
    a numerator is three float64 additions of four exact products p_i, off by at most 3u sum |p_i| (u = 2^-53,
    first order); G is three additions of positive terms, off by at most 3u G; the quotient rounds once more.
    So |N / G - x| <= (3u sum |p_i| + 3u |N|) / G + u |x| <= 7u sum |p_i| / G, 8u with the second-order terms
    (|x| G = |N| <= sum |p_i|), and the cast to float32 adds at most one float32 ulp of the component."""
    rng = np.random.default_rng(18)
    B, S, coh = 9, 33, 4
    S2 = SR.s2_of(S)
    nh = -(-S2 // coh)

    def grid(*s):
        k = rng.integers(-1023, 1024, (*s, 2)).astype(np.float32) / np.float32(1024)
        return (k[..., 0] + 1j * k[..., 1]).astype(np.complex64)
    h, x = grid(B, 1, 2, nh), grid(B, S)
    y = SR.signal32(h, x, coh)
    a0, a1 = SR.transmit(x)
    hs = h.astype(np.complex128)[:, :, :, np.arange(S2) // coh]
    assert np.array_equal(y.astype(np.complex128), hs[:, :, 0] * a0[:, None] + hs[:, :, 1] * a1[:, None])   # exact
    z, nvs = SR.combine(y, h, 0.25, S, coh)
    g = (hs[:, 0].real ** 2 + hs[:, 0].imag ** 2).sum(axis=1)[:, :S]   # 20-bit squares: exact in any order
    # sum |p_i| <= (|h0| + |h1|) (|y0| + |y1|) per part, componentwise magnitudes bounded by the moduli
    ya = np.abs(y.astype(np.complex128))[:, 0]
    pair = np.repeat(ya[:, 0::2] + ya[:, 1::2], 2, axis=1)[:, :S]
    sp = (np.abs(hs[:, 0, 0]) + np.abs(hs[:, 0, 1]))[:, :S] * pair * 2
    worst = 0.0
    for got, ref in ((z.real, x.real), (z.imag, x.imag)):
        slack = np.spacing(np.abs(ref)).astype(np.float64) + 8 * U * sp / g
        worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - ref) / slack)))
    print("worst |z - x| over its bound", worst)
    assert worst <= 1.0
    assert np.array_equal(nvs, 0.25 / g)


def test_nv_sym_is_equal_within_a_pair():
    rng = np.random.default_rng(2)
    y, h = _cn(rng, 4, 3, 24), _cn(rng, 4, 3, 2, 4)
    for nv in (0.3, 10.0 ** rng.uniform(-2, 0, 4), 10.0 ** rng.uniform(-2, 0, (4, 3))):
        _, nvs = SR.combine(y, h, nv, coh=6)
        assert np.array_equal(nvs[:, 0::2], nvs[:, 1::2]) and np.isfinite(nvs).all()
    _, nvs = SR.combine(y, h, 0.3, S=23, coh=6)
    assert nvs.shape == (4, 23) and np.array_equal(nvs[:, 0:22:2], nvs[:, 1::2])


@pytest.mark.parametrize("per_branch", [False, True])
def test_skip_and_erasure_rules(per_branch):
    rng = np.random.default_rng(3 + per_branch)
    B, S, coh = 4, 22, 6
    nh = -(-S // coh)
    y, h = _cn(rng, B, 2, S), _cn(rng, B, 2, 2, nh)
    nv = 10.0 ** rng.uniform(-2, 0, (B, 2)) if per_branch else 0.2
    for dead in (0, 1):
        hd = h.copy()
        hd[:, dead] = 0                                               # both paths of the branch: it is skipped
        k = slice(1 - dead, 2 - dead)
        alone = SR.combine(y[:, k], h[:, k], nv[:, k] if per_branch else nv, coh=coh)
        both = SR.combine(y, hd, nv, coh=coh)
        assert _bits_equal(both[0], alone[0]) and _bits_equal(both[1], alone[1])
        hi = h.copy()
        hi[:, dead, 1, 2] = np.inf                                    # an infinite gain on one path: skipped there
        got = SR.combine(y, hi, nv, coh=coh)
        sl = slice(2 * coh, 3 * coh)
        assert _bits_equal(got[0][:, sl], alone[0][:, sl]) and _bits_equal(got[1][:, sl], alone[1][:, sl])
    ho = h.copy()
    ho[:, 0, 1] = 0                                                   # one path dead: the branch still counts
    one = SR.combine(y, ho, nv, coh=coh)
    assert np.isfinite(one[1]).all() and not _bits_equal(one[0], SR.combine(y[:, 1:], h[:, 1:], nv[:, 1:] if per_branch else nv, coh=coh)[0])
    z, nvs = SR.combine(y, np.zeros_like(h), nv, coh=coh)             # no live branch: an erasure
    assert not z.any() and np.isposinf(nvs).all()


def test_nan_noise_poisons_its_row_and_a_nan_symbol_its_pair():
    y = np.ones((3, 2, 8), np.complex64)
    h = np.ones((3, 2, 2, 2), np.complex64)
    nv = np.array([[0.1, np.nan], [0.0, 0.1], [np.inf, np.inf]])
    z, nvs = SR.combine(y, h, nv, coh=4)
    assert np.isnan(z[0].real).all() and np.isnan(nvs[0]).all()       # section 10's convention, not a skip
    for r in (1, 2):                                                  # G = inf and G = 0
        assert not z[r].any() and np.isposinf(nvs[r]).all()
    y[1, 1, 5] = np.nan
    z, nvs = SR.combine(y, h, 0.1, coh=4)
    nan = np.isnan(z.real) | np.isnan(z.imag)
    assert nan[1, 4] and nan[1, 5] and nan.sum() == 2 and np.isfinite(nvs).all()


def test_equal_per_branch_noise_agrees_with_the_common_form():
    """R = 2, nv_br = nv for both branches: tests/test_mrc_ref.py's derivation, re-read for this combiner.
    A branch's term -- g_r, or a part of num0_r or num1_r, four products and three additions -- is the same
    float64 number a_r in both forms; the forms differ in what follows.  The per-branch form divides each term
    by nv (two extra roundings) before the sum.  With u = 2^-53, Sa = |a_0| + |a_1|, Sg = g_0 + g_1:
    G' nv = Sg (1 + t), |t| <= 2u (positive terms), G = Sg (1 + e), |e| <= u: nv / G and 1 / G', each rounded
    once more, differ by at most 5u relative, under 5 ulp.  The numerators may cancel, so their bound is
    absolute: |A' nv - (a_0 + a_1)| <= 2u Sa, |A - (a_0 + a_1)| <= u Sa; with the denominators' and the
    quotients' roundings the float64 quotients differ by at most 8u Sa / Sg, 9u with the second-order terms,
    and the casts to float32 add one float32 ulp."""
    rng = np.random.default_rng(14)
    B, S, nv, coh = 6, 64, 0.0371, 2
    y, h = _cn(rng, B, 2, S), _cn(rng, B, 2, 2, S // coh)
    zc, nc = SR.combine(y, h, nv, coh=coh)
    zb, nb = SR.combine(y, h, np.full((B, 2), nv), coh=coh)
    worst_nv = np.max(np.abs(nc - nb) / np.spacing(np.maximum(nc, nb)))
    h0, h1 = (h[:, :, a][:, :, np.arange(S // 2) * 2 // coh] for a in (0, 1))
    y0, y1 = y[:, :, 0::2], y[:, :, 1::2]
    f = lambda v: v.astype(np.float64)  # noqa: E731
    h0r, h0i, h1r, h1i, y0r, y0i, y1r, y1i = map(f, (h0.real, h0.imag, h1.real, h1.imag, y0.real, y0.imag, y1.real, y1.imag))
    sg = ((h0r * h0r + h0i * h0i) + (h1r * h1r + h1i * h1i)).sum(axis=1)
    terms = {(0, "real"): (y0r * h0r + y0i * h0i) + (y1r * h1r + y1i * h1i),
             (0, "imag"): (y0i * h0r - y0r * h0i) + (y1r * h1i - y1i * h1r),
             (1, "real"): (y0r * h1r + y0i * h1i) - (y1r * h0r + y1i * h0i),
             (1, "imag"): (y0i * h1r - y0r * h1i) - (y1r * h0i - y1i * h0r)}
    worst_z = 0.0
    for (odd, part), t in terms.items():
        got, ref = getattr(zb[:, odd::2], part), getattr(zc[:, odd::2], part)
        slack = np.spacing(np.maximum(np.abs(got), np.abs(ref))).astype(np.float64) + 9 * U * np.abs(t).sum(axis=1) / sg
        worst_z = max(worst_z, np.max(np.abs(got.astype(np.float64) - ref) / slack))
    print("nv_sym: worst", worst_nv, "ulp (bound 5);  z: worst", worst_z, "of its bound")
    assert worst_nv <= 5 and worst_z <= 1.0
    assert not _bits_equal(nc, nb)                                    # and it is indeed not bit for bit


def test_transmit_mapping():
    x = np.array([1 + 2j, 3 - 4j, -5 + 6j], np.complex64)
    a0, a1 = SR.transmit(x)
    assert np.array_equal(a0, np.array([1 + 2j, -3 - 4j, -5 + 6j, 0], np.complex64))
    assert np.array_equal(a1, np.array([3 - 4j, 1 - 2j, 0, -5 - 6j], np.complex64))
    # the code is orthogonal: the two slots' antenna vectors of a pair are
    m = a0[0::2] * np.conj(a0[1::2]) + a1[0::2] * np.conj(a1[1::2])
    assert not m.any()


def test_antenna_gains_extend_the_branch_draw():
    cw = np.arange(5, 9)
    g, rad = SR.gains(cw, 3, 11, 4242, K=4.0)
    assert g.shape == (4, 3, 2, 11) == rad.shape
    assert np.array_equal(g[:, :, 0], np.float64(SR.SQRT_HALF) * MR.gains(cw, 3, 11, 4242, K=4.0))
    assert not np.array_equal(g[:, :, 1], g[:, :, 0]) and not np.array_equal(g[:, 1, 1], g[:, 0, 1])
    big = SR.gains(np.arange(4096), 1, 64, 7, K=0.0)[0]
    p = np.mean(np.abs(big) ** 2, axis=(0, 1, 3))                     # E|h_a|^2 = 1/2: 262144 draws each, 1 % is > 5 sigma
    assert np.all(np.abs(p / 0.5 - 1) < 0.01)


# ---- names, refusals in front of the device, the sweep's option ------------------------------
def test_names_are_exported_and_declared():
    from modulations_amd import _native, build
    with open(os.path.join(ROOT, "include", "stbc.h")) as f:
        header = f.read()
    declared = re.findall(r"^int (\w+)\(", header, re.M)
    assert sorted(declared) == sorted(_native.STBC_EXPORTS) == ["stbc_combine_dev", "stbc_workload_dev"]
    assert not set(_native.STBC_EXPORTS) & set(_native.EXPORTS)
    assert os.path.join(ROOT, "include", "stbc.h") in build.DEPS


def test_sweep_records_the_antennas_only_when_there_are_two():
    pytest.importorskip("torch")
    from modulations_amd import ber
    ap = ber.arg_parser()
    base = ["--channel", "rayleigh", "--coherence", "106"]
    one, dflt = ap.parse_args(base + ["--tx-antennas", "1"]), ap.parse_args(base)
    assert ber.sweep_config(one) == ber.sweep_config(dflt) and "tx_antennas" not in ber.sweep_config(one)
    assert ber.channel_fading(one) == {"K": 0.0, "coh": 106}           # the call without the key: the same data
    two = ap.parse_args(base + ["--tx-antennas", "2", "--rx-branches", "2", "--llr", "int8", "--demap", "log-map",
                                "--early-stop"])
    cfg = ber.sweep_config(two)
    assert cfg["tx_antennas"] == 2 and cfg["rx_branches"] == 2 and ber.channel_fading(two)["tx_antennas"] == 2
    assert "total transmit power" in ap.format_help()
    for bad in (["--tx-antennas", "2"], base + ["--tx-antennas", "3"], base + ["--tx-antennas", "0"],
                base + ["--tx-antennas", "2", "--csi", "pilots"], base + ["--tx-antennas", "2", "--crc", "crc16"],
                base + ["--tx-antennas", "2", "--harq", "chase"],
                ["--channel", "rayleigh", "--coherence", "105", "--tx-antennas", "2"]):
        with pytest.raises(SystemExit):
            ber.main(bad)


def test_make_symbols_refuses_before_any_device_call():
    pytest.importorskip("torch")
    from modulations_amd import demap as D
    from modulations_amd import workload as W
    two = {"K": 0.0, "coh": 4, "tx_antennas": 2}
    for fading, kw in (({**two, "coh": 3}, {}), ({**two, "coh": 0}, {}), ({"K": 0.0, "tx_antennas": 2}, {}),
                       ({**two, "tx_antennas": 3}, {}), ({**two, "tx_antennas": 0}, {}),
                       (two, {"pilots": D.PilotLayout(2, 8)}), (two, {"tx": 1}), (two, {"crc": "crc16"})):
        with pytest.raises(ValueError, match="tx_antennas|transmit diversity"):
            W.make_symbols(None, 4, "QPSK", 3.0, 1, "cpu", fading=fading, **kw)


def test_combine_device_refuses_before_any_device_call():
    torch = pytest.importorskip("torch")
    from modulations_amd import demap as D
    y, h = torch.zeros((2, 2, 6), dtype=torch.complex64), torch.zeros((2, 2, 2, 3), dtype=torch.complex64)
    with pytest.raises(TypeError):
        D.stbc_combine_device(y.to(torch.complex128), h, 0.1)
    with pytest.raises(ValueError, match="3-D"):
        D.stbc_combine_device(y[0], h[0], 0.1)
    with pytest.raises(ValueError, match="even S2"):
        D.stbc_combine_device(y[:, :, :5], h, 0.1)
    with pytest.raises(ValueError, match="HIP device"):
        D.stbc_combine_device(y, h, 0.1)
