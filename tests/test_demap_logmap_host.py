"""The log-MAP soft demapper's host side (no GPU): the float64 restatement the GPU
tests compare against (tests/demap_logmap_ref.py) is checked against a
brute-force extended-precision evaluation and against the max-log formula, and
the keyword / command-line / resume-key / ABI surface exists."""
import argparse
import inspect
import os
import re

import numpy as np
import pytest

import demap_logmap_ref as R
from modulations_amd import _native, ber
from modulations_amd import demap as D
from modulations_amd import dvb_rcs2_turbo as M
from modulations_amd.workload import DevicePipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = ("BPSK", "QPSK", "8PSK", "16QAM", "64QAM", "256QAM")
NAMES = ("tdec_demap_logmap_dev", "tdec_demap_logmap", "tdec_demap_planes_logmap_dev")


def _symbols(mod, nv, n, rng):
    cons = D.constellation(mod)
    s = cons[rng.integers(0, len(cons), n)] + np.sqrt(nv / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return s.astype(np.complex64), cons


def _brute(syms, cons, bps, nv):
    """Two passes in np.longdouble, point by point: the largest exponent, then the sums."""
    ld = np.longdouble
    nv = ld(max(nv, R.NV_FLOOR))
    out = np.empty((len(syms), bps))
    for n, s in enumerate(syms):
        x = [-((ld(s.real) - ld(c.real)) ** 2 + (ld(s.imag) - ld(c.imag)) ** 2) / nv for c in cons]
        top = max(x)
        acc = [[ld(0), ld(0)] for _ in range(bps)]
        for i, xi in enumerate(x):
            for b in range(bps):
                acc[b][(i >> (bps - 1 - b)) & 1] += np.exp(xi - top)
        with np.errstate(divide="ignore"):
            out[n] = [float(np.clip(np.log(a1) - np.log(a0), -30, 30)) for a0, a1 in acc]
    return out.reshape(-1)


@pytest.mark.parametrize("mod", MODS)
def test_helper_agrees_with_extended_precision(mod):
    rng = np.random.default_rng(MODS.index(mod))
    bps = D.MODULATIONS[mod]["bps"]
    for nv in (0.001, 0.05, 0.5, 5.0):
        syms, cons = _symbols(mod, nv, 48, rng)
        got, want = R.llr(syms, cons, bps, nv), _brute(syms, cons, bps, nv)
        _, dmin = R.raw_llr(syms, cons, bps, nv)
        # float64 against longdouble: the exponents carry a relative 2^-52 of d / nv
        tol = 64 * 2.0 ** -52 * np.repeat(np.maximum(1.0, dmin / max(nv, R.NV_FLOOR)), bps)
        assert np.all(np.abs(got - want) <= tol), (mod, nv, np.max(np.abs(got - want) / tol))
        assert np.array_equal(R.llr(syms, cons, bps, nv, sign=-1), -got)


@pytest.mark.parametrize("mod", MODS)
def test_helper_equals_maxlog_where_both_saturate(mod):
    rng = np.random.default_rng(10 + MODS.index(mod))
    bps = D.MODULATIONS[mod]["bps"]
    syms, cons = _symbols(mod, 0.001, 2000, rng)
    a, b = R.llr(syms, cons, bps, 0.001), R.maxlog_llr(syms, cons, bps, 0.001)
    sat = (np.abs(a) == 30) & (np.abs(b) == 30)
    assert sat.sum() > 100
    assert np.array_equal(a[sat], b[sat])
    # and log-MAP never exceeds max-log in magnitude by more than the log of the half's size
    assert np.all(np.abs(a - b) <= np.log(len(cons)) + 1e-9)


def test_helper_nonfinite():
    cons = D.constellation("16QAM")
    s = np.array([np.nan + 0j, 1 + np.nan * 1j, np.inf + 0j, 0.3 - 0.2j], np.complex64)
    out = R.llr(s, cons, 4, 0.1).reshape(-1, 4)
    assert np.isnan(out[:3]).all() and np.isfinite(out[3]).all()


def test_keyword_surface():
    for f in (D.compute_llr, D.compute_llr_device, M.DVBRCS2_Turbo.demap_planes_device):
        p = inspect.signature(f).parameters
        assert p["algo"].default == "max-log", f
    assert inspect.signature(DevicePipeline.__init__).parameters["demap"].default == "max-log"
    for f in (D.compute_llr, D.compute_llr_device):
        with pytest.raises(ValueError, match="algo"):
            f(np.zeros(4, np.complex64), "QPSK", 0.1, algo="exact")   # refused before any device call
    assert D.check_algo("log-map") and not D.check_algo("max-log")


def test_ber_argument():
    ap = ber.arg_parser()
    assert ap.parse_args([]).demap == "max-log"
    assert ap.parse_args(["--demap", "log-map"]).demap == "log-map"
    with pytest.raises(SystemExit):
        ap.parse_args(["--demap", "exact"])


def test_ber_resume_key(tmp_path):
    def ns(**kw):
        d = dict(mod="256QAM", n=48, rate="1/3", algo="max-log", iterations=8, interleaver="valid-perm",
                 codewords=192, seed=5, early_stop=False, es_decoder="frame", demap="max-log")
        d.update(kw)
        return argparse.Namespace(**d)
    plain, lm = ber.sweep_config(ns()), ber.sweep_config(ns(demap="log-map"))
    assert "demap" not in plain                       # files of earlier sweeps keep resuming
    assert plain == ber.sweep_config(argparse.Namespace(**{k: v for k, v in vars(ns()).items() if k != "demap"}))
    assert lm == {**plain, "demap": "log-map"}
    path = str(tmp_path / "sweep.json")
    ber.save_results(path, lm, [{"ebn0_db": 1.0}])
    assert list(ber.load_resume(path, lm)) == [1.0]
    with pytest.raises(ValueError, match="another sweep"):
        ber.load_resume(path, plain)
    ber.save_results(path, plain, [{"ebn0_db": 1.0}])
    with pytest.raises(ValueError, match="another sweep"):
        ber.load_resume(path, lm)


def test_abi_names():
    src = open(os.path.join(ROOT, "include", "tdec.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTS
        assert re.search(rf"^int {name}\(", src, re.M), name
        assert "div_f32" not in re.search(rf"^int {name}\(([^;]*);", src, re.M).group(1)
