"""Every case of tests/modem_edges.py through libmodem.so (modulations_amd.modem): each kernel
instantiation mdm_fir_dev can launch, both staging branches of the mapper, the scalar and the
vector stores of the hard demodulators, the skip of k_absmax, the vector, tail and unaligned
paths of the dequantiser, and the second trip of every grid-stride loop.

Comparisons are exact: bit for bit against the numpy restatement and the C oracle.  The two
exceptions are the project's existing ones, unchanged: real-valued FIR inputs within 1e-12 of
the output scale (test_gpu_modem.close), and 8PSK decisions next to a sector boundary
(test_modem_host.psk8_boundary_ok).  tests/test_modem_edges_host.py shows on the CPU that these
inputs tell each operation from its near misses."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import modem_edges as E  # noqa: E402
from oracle import oracle as O  # noqa: E402
from modulations_amd import modem as MM  # noqa: E402
from test_gpu_modem import close  # noqa: E402
from test_modem_host import psk8_boundary_ok  # noqa: E402

C64, C128 = E.C64, E.C128


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def at_offset(a, off, dtype=torch.uint8):
    """A device copy of the array whose first byte lies `off` bytes behind a 256-byte boundary."""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.nbytes + 256, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[off:off + a.nbytes]
    view.copy_(torch.from_numpy(a.view(np.uint8).ravel()))
    return view.view(dtype)


# ---------------------------------------------------------------- FIR -------------------------
@pytest.mark.parametrize("family", E.FIR_FAMILIES)
def test_fir_integer_cases_bit_for_bit(family):
    for c in E.fir_cases(family):
        x, h = E.fir_inputs(c)
        got = MM.fir(x, h, c.up, c.down, c.offset, c.n_out)
        assert E.same_bits(got, E.fir_case_ref(c)), (c, E.fir_kernel(c))
        assert E.same_bits(got, O.modem_fir(x, h, c.up, c.down, c.offset, c.n_out)), c


def test_fir_real_inputs_vs_oracle():
    for c in E.FIR_REAL:
        x, h = E.fir_inputs(c, real=True)
        close(MM.fir(x, h, c.up, c.down, c.offset, c.n_out), O.modem_fir(x, h, c.up, c.down, c.offset, c.n_out), 1e-12)


def test_fir_device_form_equals_host_form():
    """One case per kernel of each family, into a NaN-filled output: every element is written."""
    for family in E.FIR_FAMILIES:
        seen = set()
        for c in E.fir_cases(family):
            k = E.fir_kernel(c)
            if k in seen or c.n_out <= E.n_valid(c) and family != "stride":
                continue
            seen.add(k)
            x, h = E.fir_inputs(c)
            out = torch.full((c.n_out,), float("nan"), dtype=torch.complex128, device="cuda")
            MM.fir_device(dev(x), h, c.up, c.down, c.offset, c.n_out, out=out)
            assert E.same_bits(out.cpu().numpy(), MM.fir(x, h, c.up, c.down, c.offset, c.n_out)), c
        assert seen


# ---------------------------------------------------------------- mapper ----------------------
@pytest.mark.parametrize("dt", [C64, C128])
def test_map_cases_exact(dt):
    for c in E.map_cases():
        if c.dtype != dt:
            continue
        bits, table = E.map_inputs(c)
        got = MM.map_bits(bits, c.bps, table)
        assert E.same_bits(got, E.map_ref(bits, c.bps, table)), c
        assert E.same_bits(got, O.modem_map(bits, c.bps, table)), c


@pytest.mark.parametrize("dt", [C64, C128])
def test_map_device_bits_at_byte_offsets(dt):
    """Three full blocks and a partial one: offsets 0 and 16 take the 16-byte copy on the full
    blocks, 1, 8 and 15 the byte copy."""
    for bps in range(1, 9 if dt == C64 else 8):
        c = E.MapCase(bps, dt, 3 * E.MAP_SPB * bps + bps // 2 + 1, 900 + bps)
        bits, table = E.map_inputs(c)
        ref = E.map_ref(bits, bps, table)
        for off in E.MAP_OFFSETS:
            d_bits = at_offset(bits, off)
            assert d_bits.data_ptr() % 16 == off % 16
            assert E.same_bits(MM.map_device(d_bits, bps, table).cpu().numpy(), ref), (bps, off)


@pytest.mark.parametrize("c", E.MAP_LARGE, ids=lambda c: f"bps{c.bps}")
def test_map_second_trip_of_the_block_loop(c):
    bits, table = E.map_inputs(c)
    got = MM.map_bits(bits, c.bps, table)
    assert E.same_bits(got, E.map_ref(bits, c.bps, table))
    assert E.same_bits(got, O.modem_map(bits, c.bps, table))


# ---------------------------------------------------------------- hard demodulators -----------
def _oracle(c):
    return O.modem_demod(c.syms, c.kind, c.bps, labels=c.labels, scale=c.scale, cons=c.cons,
                         nan_raises=bool(c.nan_raises))


def _device(c, out=None):
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    bits = MM.demod_device(dev(c.syms), c.kind, c.bps, labels=c.labels, scale=c.scale, cons=c.cons,
                           nan_raises=c.nan_raises, out=out, nan_count=cnt)
    return bits.cpu().numpy(), int(cnt.item())


def _host(c):
    return MM.hard_demod(c.syms, c.kind, c.bps, labels=c.labels, scale=c.scale, cons=c.cons, nan_raises=c.nan_raises)


def _check_demod(c, boundary=False):
    ref, nans = _oracle(c)
    got, cnt = _device(c)
    assert cnt == nans == E.demod_ref(c)[1], c.name
    if boundary:
        psk8_boundary_ok(c.syms, got, ref)
    else:
        assert np.array_equal(got, ref), c.name
        assert np.array_equal(got, E.demod_ref(c)[0]), c.name
    if nans:                                        # the host form reports the reference's int(NaN)
        with pytest.raises(ValueError):
            _host(c)
    else:
        assert np.array_equal(_host(c), got), c.name


@pytest.mark.parametrize("family", E.DEMOD_FAMILIES)
def test_demod_cases(family):
    for c in E.demod_cases(family):
        _check_demod(c, boundary=family == "psk8_boundary")


def test_demod_output_at_byte_offsets():
    """One store per symbol where the output is a multiple of bps, byte stores elsewhere: the same bits."""
    cases = {c.bps: c for c in E.demod_cases("qam_axis") if c.syms.dtype == C64 and "NaN" not in c.name}
    for bps, off in E.DEMOD_ALIGN:
        c = cases[bps]
        n = len(c.syms) * bps
        buf = torch.full((n + 264,), 9, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 256 == 0
        got, _ = _device(c, out=buf[off:off + n])
        assert np.array_equal(got, _oracle(c)[0]), (bps, off)
        rest = buf.cpu().numpy()
        assert (rest[:off] == 9).all() and (rest[off + n:] == 9).all(), (bps, off)


@pytest.mark.parametrize("which", ["gt0", "qam256"])
def test_demod_second_trip_of_the_grid_stride_loop(which):
    c = E.demod_large(which)
    _check_demod(c)


# ---------------------------------------------------------------- IQ formats ------------------
@pytest.mark.parametrize("dt", [C64, C128])
def test_iq_quantize_cases(dt):
    for name, sig in E.quant_cases(dt).items():
        ref = O.modem_iq_quantize(sig)
        assert np.array_equal(MM.iq_quantize(sig), ref), name
        assert np.array_equal(MM.iq_quantize_device(dev(sig)).cpu().numpy(), ref), name


def test_iq_dequantize_cases():
    for name, raw in E.dequant_cases().items():
        ref = E.dequant_ref(raw)
        assert E.same_bits(MM.iq_dequantize(raw), ref), name
        assert E.same_bits(MM.iq_dequantize_device(dev(raw)).cpu().numpy(), ref), name


def test_iq_dequantize_device_unaligned():
    """raw and out each off a 16-byte boundary: the one-by-one path; aligned again at (16, 2)."""
    for name, raw in E.dequant_cases().items():
        n = len(raw) // 2
        ref = E.dequant_ref(raw)
        for raw_off, out_off in E.DEQUANT_OFFSETS:
            buf = torch.full((n + 8,), float("nan"), dtype=torch.complex64, device="cuda")
            out = buf[out_off:out_off + n]
            d_raw = at_offset(raw, raw_off)
            assert (d_raw.data_ptr() % 16, out.data_ptr() % 16) == (raw_off % 16, 8 * out_off % 16)
            MM.iq_dequantize_device(d_raw, out=out)
            assert E.same_bits(out.cpu().numpy(), ref), (name, raw_off, out_off)
            rest = buf.cpu().numpy()
            assert np.isnan(rest[:out_off]).all() and np.isnan(rest[out_off + n:]).all()
