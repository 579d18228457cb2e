"""Flat fading, the parts that need no GPU: the ABI names, the
numpy restatements the GPU tests compare the kernels against (tests/fading_ref.py), the
erasure rule's pin in the oracle, the argument checks that refuse a tensor before any
device call, and the BER sweep's channel options."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fading_ref as F
from oracle import oracle as O
from modulations_amd import _native, ber, demap as D
from modulations_amd import dvb_rcs2_turbo as M
from modulations_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tdec_symnv_demap_dev", "tdec_symnv_demap_logmap_dev", "tdec_symnv_demap_planes_dev",
       "tdec_symnv_demap_planes_logmap_dev", "tdec_equalize_dev", "tdec_workload_fading_dev")
MODS = ["BPSK", "QPSK", "8PSK", "16QAM", "64QAM", "256QAM"]


def test_names_are_exported_and_declared():
    with open(os.path.join(ROOT, "include", "tdec.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _native.EXPORTS
        assert re.search(rf"^int {name}\(", header, re.M), name
    assert callable(D.equalize_device)


@pytest.mark.parametrize("div_f32", [False, True])
@pytest.mark.parametrize("mod", MODS)
def test_infinite_noise_variance_gives_zero_llrs(mod, div_f32):
    """The erasure rule's pin: the equaliser marks a symbol without channel knowledge with
    nv_sym = +inf, and the oracle's demap gives finite symbols all-zero LLRs there (+-0.0;
    finite meaning that the squared distances are: 1e30 overflows float32 to inf - inf)."""
    cons = D.constellation(mod)
    bps = D.MODULATIONS[mod]["bps"]
    rng = np.random.default_rng(len(mod) + div_f32)
    syms = np.concatenate([cons[rng.integers(0, len(cons), 40)] +
                           0.3 * (rng.standard_normal(40) + 1j * rng.standard_normal(40)),
                           [0.0, 1e15 - 1e15j, -3.5 + 0.25j]]).astype(np.complex64)
    llr = O.demap(syms, cons, bps, np.inf, div_f32)
    assert llr.shape == (len(syms) * bps,)
    assert np.array_equal(llr, np.zeros_like(llr))


@pytest.mark.parametrize("mod", MODS)
def test_equalised_rows_with_one_gain_demap_as_rows(mod):
    """One gain per row (coh >= S): every symbol of a row carries nv / |h|^2, so demapping
    the equalised symbols one by one with their own value is demapping the row with it."""
    cons = D.constellation(mod)
    bps = D.MODULATIONS[mod]["bps"]
    rng = np.random.default_rng(sum(map(ord, mod)))
    B, S, nv = 4, 24, 0.11
    x = cons[rng.integers(0, len(cons), (B, S))]
    h = (rng.standard_normal((B, 1)) + 1j * rng.standard_normal((B, 1))).astype(np.complex64)
    y = (h * x + 0.2 * (rng.standard_normal((B, S)) + 1j * rng.standard_normal((B, S)))).astype(np.complex64)
    for coh in (S, S + 5):
        z, nvs = F.equalize(y, h, nv, coh)
        g = h.real.astype(np.float64) ** 2 + h.imag.astype(np.float64) ** 2
        assert np.array_equal(nvs, np.broadcast_to(nv / g, (B, S)))
        np.testing.assert_allclose(z, y / h, rtol=1e-6)
        for div_f32 in (False, True):
            per_sym = F.demap_per_symbol(z, cons, bps, nvs, div_f32)
            for r in range(B):
                assert np.array_equal(per_sym[r], O.demap(z[r], cons, bps, nvs[r, 0], div_f32))


def test_equaliser_restatement_erasures_and_gain_blocks():
    y = np.array([[1 + 2j, 3 - 1j, -2 + 0.5j, 4j, 1.0]], np.complex64)
    h = np.array([[2j, 0, np.nan + 1j]], np.complex64)              # coh = 2: blocks {0, 1}, {2, 3}, {4}
    z, nvs = F.equalize(y, h, np.array([0.5]), coh=2)
    assert np.array_equal(z[0, :2], np.array([1 - 0.5j, -0.5 - 1.5j], np.complex64))   # y / 2j
    assert np.array_equal(nvs[0, :2], [0.125, 0.125])               # 0.5 / 4
    assert np.array_equal(z[0, 2:], np.zeros(3, np.complex64)) and np.all(np.isposinf(nvs[0, 2:]))
    tiny = np.array([[1e-42 + 0j]], np.complex64)                   # a denormal gain: not an erasure
    z, nvs = F.equalize(np.array([[1e-42 + 0j]], np.complex64), tiny, 1.0)
    assert z[0, 0] == 1.0 and np.isfinite(nvs[0, 0]) and nvs[0, 0] > 1e80


@pytest.mark.parametrize("K", [0.0, 4.0])
def test_gain_draw_mean_and_power(K):
    """2^18 draws: mean sqrt(K / (K + 1)) and E|h|^2 = 1 within 5 standard errors.  With
    s2 = 1 / (K + 1) the scatter's variance and a the mean, each dimension of h has
    variance s2 / 2, and |h|^2 = a^2 + 2 a Re w' + |w'|^2 has variance 2 a^2 s2 + s2^2."""
    n = 1 << 18
    h = F.gains(np.arange(1 << 8) + 12345, 1 << 10, 0xC0FFEE, K).reshape(-1)
    assert h.size == n
    a, s2 = np.sqrt(K / (K + 1.0)), 1.0 / (K + 1.0)
    se = np.sqrt(s2 / 2 / n)
    assert abs(h.real.mean() - a) < 5 * se and abs(h.imag.mean()) < 5 * se
    assert abs(np.mean(np.abs(h) ** 2) - 1.0) < 5 * np.sqrt((2 * a * a * s2 + s2 * s2) / n)
    # a gain depends on (codeword, block, seed) alone
    assert np.array_equal(F.gains([12345 + 7], 20, 0xC0FFEE, K)[0], h.reshape(1 << 8, 1 << 10)[7, :20])
    assert not np.array_equal(F.gains([12345 + 7], 20, 0xC0FFEE + 1, K)[0], h.reshape(1 << 8, 1 << 10)[7, :20])


def test_cpu_tensors_are_refused_before_any_device_call():
    syms = torch.zeros((3, 8), dtype=torch.complex64)
    nv = torch.full((3, 8), 0.05, dtype=torch.float64)
    for algo in ("max-log", "log-map"):
        with pytest.raises(ValueError):
            D.compute_llr_device(syms, "16QAM", nv, algo=algo)
    with pytest.raises(ValueError):
        D.equalize_device(syms, torch.ones((3, 8), dtype=torch.complex64), 0.1)
    c = M.DVBRCS2_Turbo(48, "1/3")
    planes = torch.zeros(16, dtype=torch.float32)
    for algo in ("max-log", "log-map"):
        with pytest.raises(ValueError, match="noise_var must be a tensor on cuda"):
            c.demap_planes_device(syms, D.constellation("16QAM"), 4, nv, planes, algo=algo)
    assert c._h is None   # no handle was made: nothing reached the device


@pytest.mark.parametrize("nv", [torch.full((3, 8), 0.05, dtype=torch.float32),          # dtype
                                torch.full((3, 7), 0.05, dtype=torch.float64),          # not [B, S]
                                torch.full((3, 16), 0.05, dtype=torch.float64)[:, ::2]])  # not contiguous
def test_wrong_dtype_or_shape_is_refused(nv):
    syms = torch.zeros((3, 8), dtype=torch.complex64)
    with pytest.raises((ValueError, TypeError)) as e:
        D.compute_llr_device(syms, "QPSK", nv)
    assert "noise_var" in str(e.value)


def test_equalize_device_checks_its_arguments():
    syms = torch.zeros((3, 8), dtype=torch.complex64)
    with pytest.raises(TypeError):
        D.equalize_device(syms.to(torch.complex128), torch.ones((3, 8), dtype=torch.complex64), 0.1)
    with pytest.raises(TypeError):
        D.equalize_device(syms, torch.ones((3, 8), dtype=torch.float32), 0.1)


class _Codec:
    """What DevicePipeline's constructor asks of a codec, without a device."""
    k_info = 96
    early_stop = False

    def fused_available(self, cons, bps):
        return True

    def reserve_fused(self, B):
        pass


def test_fused_pipeline_refuses_csi():
    pipe = W.DevicePipeline(_Codec(), "16QAM", 4, "cpu", fused=True)
    syms = torch.zeros((4, 72), dtype=torch.complex64)
    with pytest.raises(ValueError, match="fused"):
        pipe.run(syms, 0.05, csi=torch.ones((4, 72), dtype=torch.complex64))


# ---- the BER sweep's channel options ----------------------------------------------------
def _cfg(*argv):
    return ber.sweep_config(ber.arg_parser().parse_args(list(argv)))


def test_ber_channel_arguments():
    a = ber.arg_parser().parse_args([])
    assert a.channel == "awgn" and a.coherence == 1 and ber.channel_fading(a) is None
    # awgn: the configuration the parent writes, so its result files keep resuming
    assert not {"channel", "rician_k", "coherence"} & set(_cfg())
    assert _cfg("--channel", "awgn", "--rician-k", "9", "--coherence", "5") == _cfg()
    ray = _cfg("--channel", "rayleigh", "--coherence", "16", "--rician-k", "3")
    assert (ray["channel"], ray["rician_k"], ray["coherence"]) == ("rayleigh", 0.0, 16)
    ric = _cfg("--channel", "rician", "--rician-k", "2.5")
    assert (ric["channel"], ric["rician_k"], ric["coherence"]) == ("rician", 2.5, 1)
    assert {k: v for k, v in ray.items() if k not in ("channel", "rician_k", "coherence")} == _cfg()
    with pytest.raises(SystemExit):
        ber.arg_parser().parse_args(["--channel", "nakagami"])


def test_resume_with_another_channel_is_refused(tmp_path):
    path = str(tmp_path / "sweep.json")
    awgn, ray = _cfg(), _cfg("--channel", "rayleigh")
    ber.save_results(path, awgn, [{"ebn0_db": 1.0, "ber": 0.1}])
    assert list(ber.load_resume(path, awgn)) == [1.0]
    with pytest.raises(ValueError, match="channel"):
        ber.load_resume(path, ray)
    ber.save_results(path, ray, [{"ebn0_db": 2.0, "ber": 0.2}])
    assert list(ber.load_resume(path, ray)) == [2.0]
    for other in (awgn, _cfg("--channel", "rayleigh", "--coherence", "4"), _cfg("--channel", "rician")):
        with pytest.raises(ValueError):
            ber.load_resume(path, other)
