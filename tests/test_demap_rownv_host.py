"""Per-row noise variance, the parts that need no GPU: the
ABI names, the argument checks that refuse a tensor before any device call, the
fused pipeline's refusal, and the numpy restatement of the estimator that the GPU
test (tests/test_gpu_demap_rownv.py) compares the kernel against, on hand-made
rows."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import noise_var_ref as R
from modulations_amd import _native, demap as D
from modulations_amd import dvb_rcs2_turbo as M
from modulations_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tdec_noise_var_dev", "tdec_demap_rows_dev", "tdec_demap_rows_logmap_dev", "tdec_demap_planes_nv_dev",
       "tdec_demap_planes_logmap_nv_dev")


def test_names_are_exported_and_declared():
    with open(os.path.join(ROOT, "include", "tdec.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _native.EXPORTS
        assert re.search(rf"^int {name}\(", header, re.M), name
    assert callable(D.estimate_noise_var_device)


def test_cpu_tensors_are_refused_before_any_device_call():
    syms = torch.zeros((3, 8), dtype=torch.complex64)
    nv = torch.full((3,), 0.05, dtype=torch.float64)
    with pytest.raises(ValueError):
        D.estimate_noise_var_device(syms, "16QAM")
    with pytest.raises(ValueError):
        D.compute_llr_device(syms, "16QAM", nv)
    with pytest.raises(ValueError):
        D.compute_llr_device(syms, "16QAM", nv, algo="log-map")
    c = M.DVBRCS2_Turbo(48, "1/3")
    planes = torch.zeros(16, dtype=torch.float32)
    for algo in ("max-log", "log-map"):
        with pytest.raises(ValueError, match="noise_var must be a tensor on cuda"):
            c.demap_planes_device(syms, D.constellation("16QAM"), 4, nv, planes, algo=algo)
    assert c._h is None   # no handle was made: nothing reached the device


@pytest.mark.parametrize("nv", [torch.full((3,), 0.05, dtype=torch.float32),      # dtype
                                torch.full((4,), 0.05, dtype=torch.float64),      # not [B]
                                torch.full((3, 1), 0.05, dtype=torch.float64),    # not 1-D
                                torch.full((6,), 0.05, dtype=torch.float64)[::2]])  # not contiguous
def test_wrong_dtype_or_shape_is_refused(nv):
    syms = torch.zeros((3, 8), dtype=torch.complex64)
    with pytest.raises((ValueError, TypeError)) as e:
        D.compute_llr_device(syms, "QPSK", nv)
    assert "noise_var" in str(e.value)
    c = M.DVBRCS2_Turbo(48, "1/3")
    with pytest.raises((ValueError, TypeError)) as e:
        c.demap_planes_device(syms, D.constellation("QPSK"), 2, nv, torch.zeros(16, dtype=torch.float32))
    assert "noise_var" in str(e.value)
    assert c._h is None


def test_dtype_is_a_type_error_and_flat_symbols_are_refused():
    syms = torch.zeros((3, 8), dtype=torch.complex64)
    with pytest.raises(TypeError):
        D.compute_llr_device(syms, "QPSK", torch.zeros(3, dtype=torch.float32))
    with pytest.raises(ValueError, match="2-D"):
        D.compute_llr_device(syms.reshape(-1), "QPSK", torch.zeros(24, dtype=torch.float64))
    with pytest.raises(TypeError):
        D.estimate_noise_var_device(torch.zeros((3, 8), dtype=torch.complex128), "QPSK")


class _Codec:
    """What DevicePipeline's constructor asks of a codec, without a device."""
    k_info = 96
    early_stop = False

    def fused_available(self, cons, bps):
        return True

    def reserve_fused(self, B):
        pass


def test_fused_pipeline_refuses_a_tensor():
    pipe = W.DevicePipeline(_Codec(), "16QAM", 4, "cpu", fused=True)
    syms = torch.zeros((4, 72), dtype=torch.complex64)
    with pytest.raises(ValueError, match="fused"):
        pipe.run(syms, torch.full((4,), 0.05, dtype=torch.float64))


def test_estimator_restatement_on_hand_made_rows():
    cons = D.constellation("QPSK")            # complex128 table, points (+-1 +-1j) / sqrt(2)
    a = 1 / np.sqrt(2)
    rows = np.array([[a + a * 1j, -a + a * 1j, a - a * 1j, -a - a * 1j],            # on the points
                     [a + 0.5 + a * 1j, -a + (a + 0.5) * 1j, a - a * 1j, -a - a * 1j],
                     [a + a * 1j, np.nan, a - a * 1j, -a - a * 1j],
                     [a + a * 1j, np.inf, a - a * 1j, -a - a * 1j],
                     [0.0, 0.0, 0.0, 0.0]], dtype=np.complex64)                      # ties: the first label wins
    nv = R.noise_var_rows(rows, cons, 0.02)
    assert nv[0] == 0.02                      # below the floor: exactly the floor
    assert nv[1] == pytest.approx(2 * 0.25 / 4, rel=1e-6)
    assert np.isnan(nv[2]) and np.isnan(nv[3])   # a non-finite symbol: NaN, not the floor
    assert nv[4] == pytest.approx(1.0, rel=1e-6)
    # the decision is the first minimum in label order, and e_s its distance
    e = R.sq_errors(rows, cons)
    sr, si = rows.real.astype(np.float64), rows.imag.astype(np.float64)
    for r in (0, 1, 4):
        for s in range(4):
            d = [(sr[r, s] - p.real) ** 2 + (si[r, s] - p.imag) ** 2 for p in cons]
            assert e[r, s] == d[int(np.argmin(d))] == min(d)
    # Python's max(nv, floor) on the same means, NaN included
    mean = e.sum(axis=1) / 4
    for m, v in zip(mean, nv):
        py = max(float(m), 0.02)
        assert (np.isnan(py) and np.isnan(v)) or py == v
    assert R.noise_var_rows(rows[:1], cons, 0.5)[0] == 0.5
