"""The host form and the _dev form of each of libmodem.so's nine operations give the same bytes
(through modulations_amd.modem), for complex64 and complex128 samples where the operation takes
both.  The two forms share one launch path and differ in who owns the device buffers, so this is
bit for bit.  The device form writes into the front of a buffer filled with 0x5A: an element it
leaves out shows against the host form's, and every byte behind the declared length must still be
0x5A afterwards (the result records and the scratch of the receive chain included).

Shapes are the smallest that reach each branch: a bit count that is no multiple of bps, one
sample and one past a block of 256, 7 / 8 / 9 pairs around the dequantiser's vector width, two
and three tiles of the burst detector, one and three workgroups of the correlator, one candidate
and one past a carrier block of 64 (CR_BLOCK in modem_kernels.hip), with and without symbols."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulations_amd import modem as MM  # noqa: E402

FILL, PAD = 0x5A, 64
DTYPES = [np.complex64, np.complex128]
ids = dict(ids=lambda d: getattr(d, "__name__", str(d)))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """`count` elements of `dtype` at the front of a 0x5A-filled device buffer, PAD bytes behind them."""

    def __init__(self, count, dtype, shape=None):
        self.nbytes = count * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((self.nbytes + PAD,), FILL, dtype=torch.uint8, device="cuda")
        self.t = self.buf[:self.nbytes].view(dtype)
        if shape is not None:
            self.t = self.t.reshape(shape)

    def bytes(self):
        """What was written, after checking that nothing behind it was."""
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[self.nbytes:] == FILL).all(), "bytes behind the declared length were written"
        return b[:self.nbytes]


def same(g, host):
    host = np.ascontiguousarray(host)
    got = g.bytes()
    assert got.size == host.nbytes
    assert np.array_equal(got, host.view(np.uint8).ravel())


def signal(n, dtype, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) + 1j * r.standard_normal(n)).astype(dtype)


@pytest.mark.parametrize("dt", DTYPES, **ids)
def test_map(dt):
    bits = np.random.default_rng(1).integers(0, 2, 100).astype(np.uint8)      # 33 symbols and one padded bit
    table = signal(8, dt, 2)
    g = Guarded(34, torch.complex64 if dt is np.complex64 else torch.complex128)
    MM.map_device(dev(bits), 3, table, out=g.t)
    same(g, MM.map_bits(bits, 3, table))


@pytest.mark.parametrize("dt", DTYPES, **ids)
def test_demod(dt):
    syms = signal(257, dt, 3)
    g = Guarded(257 * 4, torch.uint8)
    MM.demod_device(dev(syms), MM.QAM_AXIS, 4, labels=MM._INV[2], scale=np.sqrt(10), out=g.t)
    same(g, MM.hard_demod(syms, MM.QAM_AXIS, 4, labels=MM._INV[2], scale=np.sqrt(10)))


@pytest.mark.parametrize("dt", DTYPES, **ids)
def test_fir(dt):
    x, h = signal(300, dt, 4), np.random.default_rng(5).standard_normal(5)
    g = Guarded(304, torch.complex128)
    MM.fir_device(dev(x), h, 1, 1, 0, 304, out=g.t)
    same(g, MM.fir(x, h, 1, 1, 0, 304))


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("dt", DTYPES, **ids)
def test_iq_quantize(dt, n):
    sig = signal(n, dt, 6)
    g, scratch = Guarded(2 * n, torch.int8), Guarded(1, torch.int64)
    MM.iq_quantize_device(dev(sig), out=g.t, scratch=scratch.t)
    same(g, MM.iq_quantize(sig))
    scratch.bytes()


@pytest.mark.parametrize("n_pairs", [7, 8, 9])
def test_iq_dequantize(n_pairs):
    raw = np.random.default_rng(7).integers(0, 256, 2 * n_pairs).astype(np.uint8)
    g = Guarded(n_pairs, torch.complex64)
    MM.iq_dequantize_device(dev(raw), out=g.t)
    same(g, MM.iq_dequantize(raw))


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("dt", DTYPES, **ids)
def test_mix(dt, n):
    sig = signal(n, dt, 8)
    g = Guarded(n, torch.complex128)
    MM.mix_device(dev(sig), 0.3, 2e6, dc=0.25 - 0.5j, i0=5, out=g.t)
    same(g, MM.mix(sig, 0.3, 2e6, dc=0.25 - 0.5j, i0=5))


@pytest.mark.parametrize("want_smooth", [False, True])
@pytest.mark.parametrize("n", [1025, 2049])
@pytest.mark.parametrize("dt", DTYPES, **ids)
def test_burst_find(dt, n, want_smooth):
    sig = 0.05 * signal(n, dt, 9)
    sig[700:900] += 1
    dc = np.mean(sig)
    start, mx, smooth = MM.burst_find(sig, 8, win=16, dc=dc, want_smooth=want_smooth)
    assert start >= 0
    res, scratch = Guarded(2, torch.int64), Guarded(2 * -(-n // 1024), torch.int64)
    sm = Guarded(n, torch.float64) if want_smooth else None
    MM.burst_find_device(dev(sig), 8, win=16, dc=dc, smooth=sm.t if sm else None, result=res.t, scratch=scratch.t)
    got = res.bytes()
    assert int(got.view(np.int64)[0]) == start and got[8:].view(np.float64)[0] == mx
    assert MM.burst_result(res.t) == (start, mx)
    scratch.bytes()
    if sm:
        same(sm, smooth)


@pytest.mark.parametrize("want_corr", [False, True])
@pytest.mark.parametrize("n_region", [1031, 2056])
def test_xcorr_peak(n_region, want_corr):
    region, wave = signal(n_region, np.complex128, 10), signal(8, np.complex128, 11)
    n_out = n_region - 8 + 1
    idx, peak, corr = MM.xcorr_peak(region, wave, want_corr=want_corr)
    res, scratch = Guarded(2, torch.int64), Guarded(2 * -(-n_out // 1024), torch.int64)
    co = Guarded(n_out, torch.float64) if want_corr else None
    MM.xcorr_peak_device(dev(region), dev(wave), corr=co.t if co else None, result=res.t, scratch=scratch.t)
    got = res.bytes()
    assert got[:8].view(np.float64)[0] == peak and int(got[8:].view(np.int64)[0]) == idx
    assert MM.xcorr_result(res.t) == (idx, peak)
    scratch.bytes()
    if co:
        same(co, corr)


@pytest.mark.parametrize("n", [0, 8])
@pytest.mark.parametrize("n_cand", [1, 65])
def test_carrier(n_cand, n):
    r = np.random.default_rng(12)
    syms = signal(n_cand * n, np.complex128, 13).reshape(n_cand, n)
    ph, fr = r.uniform(-3, 3, n_cand), r.uniform(-0.1, 0.1, n_cand)
    al, kd = r.uniform(0.001, 0.05, n_cand), r.integers(0, 3, n_cand).astype(np.int32)
    out, fin = MM.carrier_recovery(syms, ph, fr, al, kd)
    g_out = Guarded(n_cand * n, torch.complex128, (n_cand, n))
    g_fin = Guarded(n_cand * 2, torch.float64, (n_cand, 2))
    MM.carrier_recovery_device(dev(syms), ph, fr, al, kd, out=g_out.t, final=g_fin.t)
    same(g_out, out)
    same(g_fin, fin)
