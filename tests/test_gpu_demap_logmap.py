"""The log-MAP (exact log-sum) soft demapper on the GPU:
tdec_demap_logmap_dev / tdec_demap_logmap / tdec_demap_planes_logmap_dev and the
Python surface above them.

Accuracy is against the float64 restatement of the definition over all M points
(tests/demap_logmap_ref.py), never against the kernel itself, with the bound

    |err| <= c * eps * max(1, d_min / nv),   eps = 2^-23 (f32 arithmetic) or 2^-52 (f64)

where d_min is the symbol's smallest squared distance and c = 2 * C_MEASURED:
C_MEASURED = 78 is the smallest integer that held over exactly these inputs when the
kernels were first run (worst ratio 77.27; the figures per table are in DESIGN.md section 9),
the factor 2 is for symbols drawn with other seeds.  The separable route (square
16 / 64 / 256QAM) and the full scan (BPSK, QPSK, 8PSK, a rotated 16QAM and a
256QAM table made non-separable by one ulp) answer to the same bound.
Everything else is an exact relation (IEEE ==)."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("trans_tables")]

import demap_logmap_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402
from modulations_amd import _native as _n  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd.workload import DevicePipeline, count_errors, make_symbols  # noqa: E402

C_MEASURED = 78   # worst ratio 77.27: 16QAM rotated by 0.1 rad, nv = 0.05, the flat kernel on 4 099 symbols
MODS = ("BPSK", "QPSK", "8PSK", "16QAM", "64QAM", "256QAM")
N_SYMS = (1, 63, 64, 65, 257, 4099)
NVS = (0.001, 0.005, 0.05, 0.5, 5.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _table(name):
    """(label-ordered table, bps): the built-in ones, 16QAM rotated by 0.1 rad
    (not separable: the full scan over 16 points) and 256QAM with one coordinate
    moved by one ulp (not separable: the full scan over 256 points)."""
    if name == "16QAM-rot":
        return (D.constellation("16QAM").astype(np.complex128) * np.exp(0.1j)).astype(np.complex64), 4
    if name == "256QAM-scan":
        c = D.constellation("256QAM").copy()
        c[37] = np.nextafter(c[37].real, np.float32(9)) + 1j * c[37].imag
        return c, 8
    return D.constellation(name), D.MODULATIONS[name]["bps"]


TABLES = MODS + ("16QAM-rot", "256QAM-scan")


def _symbols(cons, n, nv, rng, f64=False):
    """Table points plus complex Gaussian noise of variance nv; from 63 symbols
    up, four exactly on decision boundaries (midpoints of nearest neighbours) and
    four far outside the grid."""
    c = cons.astype(np.complex128)
    s = c[rng.integers(0, len(c), n)] + np.sqrt(nv / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if n >= 63:
        i = rng.integers(0, len(c), 4)
        d = np.abs(c[i, None] - c[None, :])
        d[np.arange(4), i] = np.inf
        s[:4] = (c[i] + c[d.argmin(axis=1)]) / 2
        r = np.abs(c).max()
        s[4:8] = r * np.array([3, 3, 10, 10]) * np.exp(2j * np.pi * rng.random(4))
    return s if f64 else s.astype(np.complex64)


def _flat_dev(syms, cons, bps, nv, sign=+1):
    """tdec_demap_logmap_dev over any table (numpy in, numpy out)."""
    s64 = syms.dtype == np.complex128
    f64 = s64 or cons.dtype == np.complex128
    c = np.ascontiguousarray(cons.astype(np.complex128 if f64 else np.complex64))
    d_s = torch.from_numpy(np.ascontiguousarray(syms)).cuda()
    out = torch.empty(len(syms) * bps, dtype=torch.float64, device="cuda")
    _n.check(_n.lib().tdec_demap_logmap_dev(0, _n.ptr(d_s), int(s64), len(syms), _n.ptr(c), int(f64), len(c), bps,
                                            float(nv), int(sign), _n.ptr(out),
                                            torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


_CODEC = {}


def _codec(N=48, rate="1/3", algo="max-log"):
    k = (N, rate, algo)
    if k not in _CODEC:
        _CODEC[k] = M.DVBRCS2_Turbo(N, rate, algo=algo, interleaver="valid-perm", device=0)
    return _CODEC[k]


_MAP = {}


def _plane_map(c, B):
    """int64 [planes]: 1 + (row * llr_len + j) of the LLR a plane entry holds, 0 for an
    entry no LLR feeds -- the de-puncture kernel run over the LLRs' own indices."""
    k = (id(c), B)
    if k not in _MAP:
        L = c.handle.llr_len
        assert B * L < 2 ** 24                        # exact in f32
        idx = (1 + np.arange(B * L, dtype=np.float32)).reshape(B, L)
        planes = torch.zeros(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
        c.reserve(B)
        c.depuncture_device(torch.from_numpy(idx).cuda(), planes)
        _MAP[k] = planes.cpu().numpy().astype(np.int64)
    return _MAP[k]


def _planes_dev(c, syms2d, cons, bps, nv, algo="log-map"):
    B = syms2d.shape[0]
    c.reserve(B)
    planes = torch.full((c.planes_bytes(B) // 4,), 7.0, dtype=torch.float32, device="cuda")
    c.demap_planes_device(torch.from_numpy(np.ascontiguousarray(syms2d)).cuda(), cons, bps, nv, planes, algo=algo)
    return planes


def _rows_from_planes(c, planes, B):
    """float32 [B, llr_len] read back through the plane map (0 where no entry holds the LLR)."""
    pm = _plane_map(c, B)
    out = np.zeros(B * c.handle.llr_len + 1, np.float32)
    out[pm] = planes.cpu().numpy()[:len(pm)]
    return out[1:].reshape(B, -1)


def _judge(got, syms, cons, bps, nv, eps, sign):
    """(worst |err| / (eps * max(1, d_min / nv)), entries neither side clips).  The ratio
    is taken over every entry: one that only one side clips is then held to the same
    bound around +-30, and one both sides clip has no error."""
    raw, dmin = R.raw_llr(syms, cons, bps, nv)
    want = sign * np.clip(raw, -30, 30).reshape(-1)
    unit = eps * np.repeat(np.maximum(1.0, dmin / max(nv, R.NV_FLOOR)), bps)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    ratio = np.abs(got - want) / unit
    clipped = (np.abs(got) == 30) | (np.abs(want) == 30)
    return float(ratio.max(initial=0.0)), int((~clipped).sum())


def _worse(worst, r, at):
    return (r, at) if r > worst[0] else worst


# ---- accuracy ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLES)
def test_accuracy_against_the_float64_definition(name):
    cons, bps = _table(name)
    rng = np.random.default_rng(100 + TABLES.index(name))
    c = _codec()
    L = c.handle.llr_len
    S = -(-L // bps)
    f64_table = cons.dtype == np.complex128
    worst, seen = (0.0, None), 0
    for nv in NVS:
        for n in N_SYMS:
            syms = _symbols(cons, n, nv, rng)
            # the flat kernel, both signs' arithmetic being the same: reference sign
            r, k = _judge(_flat_dev(syms, cons, bps, nv), syms, cons, bps, nv, 2.0 ** (-52 if f64_table else -23), +1)
            worst, seen = _worse(worst, r, ("flat", nv, n)), seen + k
            # the plane kernel: the same symbols as rows of S (zero symbols fill the last row)
            B = -(-n // S)
            pad = np.zeros(B * S, np.complex64)
            pad[:n] = syms
            planes = _planes_dev(c, pad.reshape(B, S), cons, bps, nv)
            rows = _rows_from_planes(c, planes, B).astype(np.float64)
            m = min(L, S * bps)
            pm = _plane_map(c, B)
            held = np.zeros(B * L + 1, bool)
            held[pm] = True                                    # LLRs some plane entry holds (not punctured)
            held = held[1:].reshape(B, L)[:, :m]
            wsyms = pad.reshape(B, S)
            raw, dmin = R.raw_llr(wsyms.reshape(-1), cons, bps, nv)
            want = -np.clip(raw, -30, 30).reshape(B, S * bps)[:, :m]
            unit = (2.0 ** -23) * np.repeat(np.maximum(1.0, dmin / max(nv, R.NV_FLOOR)), bps).reshape(B, -1)[:, :m]
            if f64_table:   # f64 arithmetic rounded to f32 planes: the rounding is the plane format's
                unit = 2.0 ** -52 / 2.0 ** -23 * unit
                slack = np.abs(want) * 2.0 ** -24
            else:
                slack = 0.0
            got = rows[:, :m]
            err = np.maximum(0.0, np.abs(got - want) - slack)[held]
            r = float((err / unit[held]).max(initial=0.0))
            worst = _worse(worst, r, ("planes", nv, n))
    # complex128 symbols: f64 arithmetic whatever the table
    for nv in (0.005, 0.5):
        syms = _symbols(cons, 257, nv, rng, f64=True)
        r, k = _judge(_flat_dev(syms, cons, bps, nv, sign=-1), syms, cons, bps, nv, 2.0 ** -52, -1)
        worst = _worse(worst, r, ("flat-f64", nv, 257))
    print(json.dumps({"table": name, "worst_ratio": worst[0], "at": worst[1], "unclipped_flat_entries": seen}))
    assert seen > 1000
    assert worst[0] <= 2 * C_MEASURED, (name, worst)


# ---- exact relations -----------------------------------------------------------------------
@pytest.mark.parametrize("mod", MODS)
def test_sign_and_host_pointer_forms(mod):
    cons, bps = _table(mod)
    rng = np.random.default_rng(7)
    syms = _symbols(cons, 4099, 0.05, rng)
    d = torch.from_numpy(syms).cuda()
    pos = D.compute_llr_device(d, mod, 0.05, algo="log-map").cpu().numpy()
    neg = D.compute_llr_device(d, mod, 0.05, sign=-1, algo="log-map").cpu().numpy()
    assert np.array_equal(neg, -pos)
    assert np.array_equal(D.compute_llr(syms, mod, 0.05, algo="log-map"), pos)
    assert np.array_equal(D.compute_llr(syms, mod, 0.05, sign=-1, algo="log-map"), neg)
    assert np.array_equal(_flat_dev(syms, cons, bps, 0.05), pos)
    # and it is not the max-log demapper
    assert not np.array_equal(D.compute_llr_device(d, mod, 0.05).cpu().numpy(), pos)
    with pytest.raises(ValueError, match="algo"):
        D.compute_llr_device(d, mod, 0.05, algo="exact")


@pytest.mark.parametrize("name", ["8PSK", "16QAM", "256QAM", "16QAM-rot"])
def test_nan_symbol_poisons_its_own_bits_only(name):
    cons, bps = _table(name)
    rng = np.random.default_rng(8)
    syms = _symbols(cons, 300, 0.05, rng)
    bad = {5: np.nan + 0j, 64: 0.1 + np.nan * 1j, 130: np.nan * (1 + 1j), 131: np.inf + 0j, 299: 0.2 - np.inf * 1j}
    for i, v in bad.items():
        syms[i] = v
    out = _flat_dev(syms, cons, bps, 0.05).reshape(-1, bps)
    want = np.zeros(300, bool)
    want[list(bad)] = True
    assert np.array_equal(np.isnan(out), np.repeat(want[:, None], bps, axis=1))
    c = _codec()
    S = -(-c.handle.llr_len // bps)
    B = 300 // S
    rows = _rows_from_planes(c, _planes_dev(c, syms[:B * S].reshape(B, S), cons, bps, 0.05), B)
    flat = (-out[:B * S]).astype(np.float32).reshape(B, S * bps)[:, :c.handle.llr_len]
    pm = _plane_map(c, B)
    held = np.zeros(B * c.handle.llr_len + 1, bool)
    held[pm] = True
    held = held[1:].reshape(B, -1)[:, :flat.shape[1]]
    assert np.array_equal(rows[:, :flat.shape[1]][held], flat[held], equal_nan=True)


SHAPES = [(48, "1/3", "256QAM", 36), (48, "1/3", "256QAM", 35), (48, "1/3", "256QAM", 37),
          (48, "1/2", "8PSK", 64), (212, "1/3", "16QAM", 318), (48, "2/3", "64QAM", None)]


@pytest.mark.parametrize("B", [1, 63, 65, 200])
@pytest.mark.parametrize("N,rate,mod,S", SHAPES)
def test_planes_equal_flat_demap_then_depuncture(N, rate, mod, S, B):
    c = _codec(N, rate)
    cons, bps = _table(mod)
    L = c.handle.llr_len
    if S is None:
        S = -(-L // bps)
    if (N, mod, S) == (48, "256QAM", 36):
        assert S * bps == L                            # the exact fit; 35 pads with zeros, 37 is truncated
    rng = np.random.default_rng(B)
    syms = _symbols(cons, B * S, 0.05, rng).reshape(B, S)
    planes = _planes_dev(c, syms, cons, bps, 0.05)
    llr = D.compute_llr_device(torch.from_numpy(syms).cuda(), mod, 0.05, sign=-1, algo="log-map")
    rows = torch.zeros((B, L), dtype=torch.float32, device="cuda")
    m = min(L, S * bps)
    rows[:, :m] = llr.to(torch.float32).reshape(B, S * bps)[:, :m]
    ref = torch.full_like(planes, 7.0)
    c.depuncture_device(rows, ref)
    assert torch.equal(planes, ref)


def test_batch_split_at_any_row():
    c = _codec()
    cons, bps = _table("256QAM")
    B, S, L = 200, 36, c.handle.llr_len
    syms = _symbols(cons, B * S, 0.5, np.random.default_rng(3)).reshape(B, S)
    whole = _rows_from_planes(c, _planes_dev(c, syms, cons, bps, 0.5), B)
    for r in (1, 63, 64, 65, 137, 199):
        a = _rows_from_planes(c, _planes_dev(c, syms[:r], cons, bps, 0.5), r)
        b = _rows_from_planes(c, _planes_dev(c, syms[r:], cons, bps, 0.5), B - r)
        assert np.array_equal(np.concatenate([a, b]), whole), r
    assert L == whole.shape[1]


def test_argument_errors():
    c = _codec()
    cons, bps = _table("16QAM")
    tab = np.ascontiguousarray(cons)
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda")
    L = _n.lib()
    assert L.tdec_demap_logmap_dev(0, None, 0, 4, _n.ptr(tab), 0, 16, 4, 0.1, 1, _n.ptr(buf), None) == _n.TDEC_EINVAL
    assert L.tdec_demap_logmap_dev(0, _n.ptr(buf), 0, 4, _n.ptr(tab), 0, 17, 4, 0.1, 1, _n.ptr(buf), None) == _n.TDEC_EINVAL
    assert L.tdec_demap_logmap_dev(0, _n.ptr(buf), 0, 4, _n.ptr(tab), 0, 16, 9, 0.1, 1, _n.ptr(buf), None) == _n.TDEC_EINVAL
    assert L.tdec_demap_logmap_dev(0, _n.ptr(buf), 0, -1, _n.ptr(tab), 0, 16, 4, 0.1, 1, _n.ptr(buf), None) == _n.TDEC_EINVAL
    assert L.tdec_demap_logmap_dev(0, _n.ptr(buf), 0, 0, _n.ptr(tab), 0, 16, 4, 0.1, 1, _n.ptr(buf), None) == 0
    host = np.zeros(8, np.complex64)
    assert L.tdec_demap_logmap(0, _n.ptr(host), 0, 8, None, 0, 16, 4, 0.1, 1, _n.ptr(np.zeros(32))) == _n.TDEC_EINVAL
    h = c.handle.h
    assert L.tdec_demap_planes_logmap_dev(None, 1, _n.ptr(buf), 36, _n.ptr(tab), 0, 16, 4, 0.1, _n.ptr(buf), None) \
        == _n.TDEC_EINVAL
    assert L.tdec_demap_planes_logmap_dev(h, 1, _n.ptr(buf), 0, _n.ptr(tab), 0, 16, 4, 0.1, _n.ptr(buf), None) \
        == _n.TDEC_EINVAL
    assert L.tdec_demap_planes_logmap_dev(h, 1, None, 36, _n.ptr(tab), 0, 16, 4, 0.1, _n.ptr(buf), None) == _n.TDEC_EINVAL
    assert L.tdec_demap_planes_logmap_dev(h, 0, None, 36, _n.ptr(tab), 0, 16, 4, 0.1, None, None) == 0
    with pytest.raises(ValueError, match="algo"):
        c.demap_planes_device(buf, cons, 4, 0.1, buf, algo="exact")


# ---- chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["max-log", "log-map"])
def test_pipeline_chain_against_the_oracle(algo):
    dev = torch.device("cuda", 0)
    c = _codec(48, "1/3", algo)
    B = 200
    _, syms, n0 = make_symbols(c, B, "256QAM", 6.0, 21, dev, want_info=False)
    pipe = DevicePipeline(c, "256QAM", B, dev, demap="log-map")
    bits = pipe.run(syms, n0).clone()
    _, _, nve = D.demap_mode(np.complex64, D.constellation("256QAM").dtype, np.float64(n0))
    llr = D.compute_llr_device(syms, "256QAM", nve, sign=-1, algo="log-map").to(torch.float32)
    L = c.handle.llr_len
    rows = llr.reshape(B, -1)[:, :L].cpu().numpy()
    assert rows.shape[1] == L
    t, _ = O.trellis()
    want = O.decode_batch(rows, c.N, c.punct["period"], T.puncture_matrix(c.punct), c.iterations, c.perm, c.inv_perm,
                          t, algo=int(algo == "log-map"), nthreads=16)
    assert np.array_equal(bits.cpu().numpy(), want)
    # demap="max-log" is the default pipeline, bit for bit; fused + log-map runs the two launches
    d0 = DevicePipeline(c, "256QAM", B, dev).run(syms, n0).clone()
    d1 = DevicePipeline(c, "256QAM", B, dev, demap="max-log").run(syms, n0).clone()
    assert torch.equal(d0, d1)
    pf = DevicePipeline(c, "256QAM", B, dev, fused=True, demap="log-map")
    assert pf.fused is False
    assert torch.equal(pf.run(syms, n0), bits)
    with pytest.raises(ValueError, match="algo"):
        DevicePipeline(c, "256QAM", B, dev, demap="exact")


# ---- sweep ---------------------------------------------------------------------------------
def test_ber_sweep_with_the_logmap_demapper(tmp_path):
    from modulations_amd import ber
    out = tmp_path / "lm.json"
    args = ["--mod", "256QAM", "--n", "48", "--rate", "1/3", "--interleaver", "valid-perm", "--ebn0", "5",
            "--codewords", "320", "--batch", "192", "--seed", "5", "--demap", "log-map", "--out", str(out)]
    rec, = ber.main(args)
    doc = json.loads(out.read_text())
    assert doc["config"]["demap"] == "log-map" and doc["points"][0]["demap"] == "log-map"
    assert rec["codewords"] == 320
    dev = torch.device("cuda", 0)
    c = _codec()
    seed = ber.ebn0_seed(5, 5.0)
    _, syms, n0 = make_symbols(c, 320, "256QAM", 5.0, seed, dev, want_info=False)
    pipe = DevicePipeline(c, "256QAM", 320, dev, demap="log-map")
    e = count_errors(c, pipe.run(syms, n0), seed)
    assert int(e.sum()) == rec["bit_errors"] and int((e > 0).sum()) == rec["frame_errors"]
    with pytest.raises(SystemExit):   # the other demapper into the same file is another sweep
        ber.main([a for a in args if a not in ("--demap", "log-map")])
