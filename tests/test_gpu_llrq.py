"""Quantised channel LLRs on the device (include/llrq.h).

Every comparison is bit for bit on the raw bytes: the quantiser against its numpy restatement
(tests/llrq_ref.py), the narrow-row de-puncture and soft-combining kernels against the float32
kernels on the rows the restatement widens, the narrow decode entry points against
decode_device of the widened rows, the host-pointer call against the device one, the
pipeline's soft-bit link against its three calls made by hand, and the refusals.

Shapes are the smallest that can go wrong: N = 48 at every rate and N = 212 at rate 2/3 (3
does not divide 212), 1 / 63 / 64 / 65 / 130 codewords (tile boundary, ragged last tile),
strides and bases that leave no row aligned, lengths around the quantiser's 16-byte vector."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import llrq_ref as Q  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

CODES = [(48, "1/3"), (48, "1/2"), (48, "2/3"), (48, "3/4"), (212, "2/3")]
BATCHES = (1, 63, 64, 65, 130)
STEPS = (np.float32(0.25), np.float32(0.3))          # a power of two and not one
GUARD = 64
SENTINEL = 12345.678      # no int8 multiple of either step, no float16 value
F16_SPECIALS = np.array([np.inf, -np.inf, np.nan, 65504.0, -65504.0, 6e-8, -6e-8, -0.0], np.float16)
Q_SPECIALS = np.float32([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -126.5, 127.5, -127.5, np.inf, -np.inf, np.nan,
                         -0.0, 0.0, 127.0, -127.0, 128.0, 1e30, -1e-45])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _codec(n, rate, **kw):
    return M.DVBRCS2_Turbo(n, rate, interleaver="valid-perm", **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(t):
    """The tensor's bytes as a numpy array (NaN payloads and signed zeros compare as bits)."""
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def _narrow_rows(rng, kind, B, L):
    """[B, L] narrow rows with the edge values of their kind sprinkled in."""
    if kind == "int8":
        q = rng.integers(-128, 128, (B, L)).astype(np.int8)
        q.flat[rng.integers(0, q.size, max(3, q.size // 16))] = rng.choice(np.int8([-128, 127, 0]), max(3, q.size // 16))
        q.flat[:3] = np.int8([-128, 127, 0])
        return q
    x = (rng.standard_normal((B, L)) * 8).astype(np.float16)
    at = rng.integers(0, x.size, max(8, x.size // 16))
    x.flat[at] = F16_SPECIALS[rng.integers(0, len(F16_SPECIALS), len(at))]
    x.flat[:len(F16_SPECIALS)] = F16_SPECIALS[:min(len(F16_SPECIALS), x.size)]
    return x


def _widen(kind, rows, step):
    return Q.dequantize_i8(rows, step) if kind == "int8" else Q.dequantize_f16(rows)


def _strided(rows, stride, offset):
    """The rows on the device `stride` elements apart behind `offset` leading elements: a [B, L] view."""
    B, L = rows.shape
    flat = torch.zeros(offset + B * stride, dtype=torch.from_numpy(rows[:1, :1]).dtype, device="cuda")
    view = torch.as_strided(flat, (B, L), (stride, 1), offset)
    view.copy_(torch.from_numpy(rows))
    return view


def _planes(c, B, fill):
    n = c.planes_bytes(B) // 4 + GUARD
    if isinstance(fill, float):
        return torch.full((n,), fill, dtype=torch.float32, device="cuda")
    return _dev(fill(n))


KINDS = [("int8", s) for s in STEPS] + [("f16", None)]


# ---- 1. the quantiser against the restatement ------------------------------------------------------

@pytest.mark.parametrize("f64", [False, True])
def test_quantizer_matches_the_restatement(f64):
    rng = np.random.default_rng(5 + f64)
    dt = np.float64 if f64 else np.float32
    tie64 = np.float64(2.5) + np.float64(2.0) ** -30          # a tie only after its float32 rounding
    for step in (np.float32(1), Q.DEFAULT_STEP, np.float32(0.3)):
        for n in (1, 15, 16, 17, 63, 64, 65, 4099):
            x = (rng.standard_normal(n) * 60 * float(step)).astype(dt)
            sp = (Q_SPECIALS * step).astype(dt)
            if f64:
                sp = np.concatenate([sp, [tie64 * float(step) if step == 1 else tie64]])
            at = rng.permutation(n)[:min(n, len(sp))]
            x[at] = sp[:len(at)]
            for off_in in (0, 1, 2, 3):
                for off_out in (0, 1, 2, 3):
                    src = torch.zeros(n + off_in, dtype=torch.float64 if f64 else torch.float32, device="cuda")
                    src[off_in:] = torch.from_numpy(x)
                    dst = torch.full((n + off_out + GUARD,), 99, dtype=torch.int8, device="cuda")
                    sat = torch.full((1,), 1000, dtype=torch.int64, device="cuda")
                    got, cnt = D.quantize_llr_device(src[off_in:], step, out=dst[off_out:off_out + n],
                                                     count_saturated=sat)
                    want = np.full(n + off_out + GUARD, 99, np.int8)
                    want[off_out:off_out + n] = Q.quantize(x, step)
                    assert np.array_equal(_raw(dst), want.view(np.uint8)), (float(step), n, off_in, off_out)
                    assert cnt is sat and int(sat.item()) == 1000 + Q.saturated(x, step), (float(step), n)
    # a fresh counter, and no counter: the quantiser then touches nothing but its output
    x = np.float32([1e9, -1e9, np.inf, 3.0, np.nan])
    q, cnt = D.quantize_llr_device(_dev(x), np.float32(1), count_saturated=True)
    assert int(cnt.item()) == 3 and np.array_equal(q.cpu().numpy(), Q.quantize(x, np.float32(1)))
    q = D.quantize_llr_device(_dev(x.reshape(5, 1)), np.float32(1))
    assert isinstance(q, torch.Tensor) and q.shape == (5, 1) and q.dtype == torch.int8


# ---- 2. the narrow de-puncture against the float32 kernel on the widened rows ----------------------

@pytest.mark.parametrize("n,rate", CODES)
def test_depuncture_matches_the_float_kernel_on_the_widened_rows(n, rate):
    c = _codec(n, rate)
    L = c.handle.llr_len
    rng = np.random.default_rng([n, CODES.index((n, rate))])
    for kind, step in KINDS:
        for B in BATCHES:
            rows = _narrow_rows(rng, kind, B, L)
            ref = _planes(c, B, SENTINEL)
            c.depuncture_device(_dev(_widen(kind, rows, step)), ref)
            assert not bool((ref[:c.planes_bytes(B) // 4] == np.float32(SENTINEL)).any())      # lanes past B are written too
            for stride in (L, L + 1, L + 3):
                for offset in (0, 1):
                    got = _planes(c, B, SENTINEL)
                    c.depuncture_device(_strided(rows, stride, offset), got, llr_step=step)
                    assert np.array_equal(_raw(got), _raw(ref)), (kind, step, B, stride, offset)


# ---- 3. the narrow soft combining against harq_depuncture_acc_dev ----------------------------------

@pytest.mark.parametrize("rv", [0, 1])
def test_accumulate_matches_the_float_kernel_on_the_widened_rows(rv):
    c = _codec(48, "1/2", rv=rv)
    L, n_slots = c.handle.llr_len, 130
    rng = np.random.default_rng(40 + rv)
    perm = rng.permutation(n_slots).astype(np.int32)
    holes = rng.integers(0, n_slots, n_slots).astype(np.int32)
    holes[[0, 5, 64, 129]] = [-1, n_slots, -1, n_slots + 7]
    few = rng.integers(0, 40, n_slots).astype(np.int32)
    maps = [("null", n_slots, None), ("perm", n_slots, perm), ("holes", n_slots, holes), ("few", 40, few)]
    start = (rng.standard_normal(c.planes_bytes(n_slots) // 4 + GUARD) * 4).astype(np.float32)
    for kind, step in KINDS:
        for name, n_rows, row_of in maps:
            rows = _narrow_rows(rng, kind, n_rows, L)
            r = None if row_of is None else _dev(row_of)
            ref, got = _dev(start), _dev(start)
            c.depuncture_accumulate_device(_dev(_widen(kind, rows, step)), ref, n_slots, row_of=r)
            c.depuncture_accumulate_device(_strided(rows, L + 3, 1), got, n_slots, row_of=r, llr_step=step,
                                           f16=kind == "f16")
            assert np.array_equal(_raw(got), _raw(ref)), (kind, step, name)
            assert not np.array_equal(_raw(got), start.view(np.uint8))
            if name == "holes":   # the slots without a row: byte-identical before and after
                T, g = 48 * 64 * 6, got.cpu().numpy().view(np.uint32)
                s0 = start.view(np.uint32)
                for slot in (0, 5, 64, 129):
                    tile, lane = divmod(slot, 64)
                    for a, w in ((tile * T, 4), (tile * T + 48 * 64 * 4, 2)):
                        assert np.array_equal(g[a:a + 48 * 64 * w].reshape(48, 64, w)[:, lane],
                                              s0[a:a + 48 * 64 * w].reshape(48, 64, w)[:, lane]), slot


# ---- 4. decode parity ---------------------------------------------------------------------------------

def _noisy_llrs(c, B, seed, amp=1.6):
    """LLR rows of random codewords at a noise level where early stop's counts differ by row."""
    rng = np.random.default_rng(seed)
    coded = c.encode_batch(rng.integers(0, 2, (B, c.k_info)).astype(np.int32))
    return ((1.0 - 2.0 * coded) * amp + rng.standard_normal(coded.shape) * 1.4).astype(np.float32)


_LLRS = {}


def _llrs(n, rate, B=130):
    if (n, rate, B) not in _LLRS:
        x = _noisy_llrs(_codec(n, rate), B, [n, B])
        x.setflags(write=False)
        _LLRS[n, rate, B] = x
    return _LLRS[n, rate, B]


@pytest.mark.parametrize("decoder", [None, "frame", "tile", "refill"])
@pytest.mark.parametrize("algo", ["max-log", "log-map"])
@pytest.mark.parametrize("n,rate", [(48, "1/2"), (212, "2/3")])
def test_decode_device_matches_the_widened_rows(n, rate, algo, decoder):
    kw = {} if decoder is None else {"early_stop": True, "es_decoder": decoder}
    c = _codec(n, rate, algo=algo, **kw)
    B, x = 130, _llrs(n, rate)
    narrow = [("int8", Q.DEFAULT_STEP, Q.quantize(x)), ("int8", np.float32(0.3), Q.quantize(x, np.float32(0.3))),
              ("f16", None, x.astype(np.float16))]
    for kind, step, rows in narrow:
        def run(t, **k):
            bits = torch.empty((B, c.k_info), dtype=torch.int32, device="cuda")
            lf = torch.empty((B, c.k_info), dtype=torch.float64, device="cuda")
            ni = torch.full((B,), -1, dtype=torch.int32, device="cuda") if decoder else None
            c.decode_device(t, bits=bits, lfinal=lf, n_iter=ni, **k)
            return _raw(bits), _raw(lf), None if ni is None else ni.cpu().numpy()
        want = run(_dev(_widen(kind, rows, step if step is not None else 1)))
        got = run(_strided(rows, rows.shape[1] + 3, 1), llr_step=step)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (kind, step)
        if decoder:
            assert np.array_equal(got[2], want[2]) and got[2].min() >= 1
    if decoder:
        assert len(set(want[2].tolist())) > 1      # the rows do stop at different counts


# ---- 5. host parity -----------------------------------------------------------------------------------

def _device_result(c, q, step):
    B = q.shape[0]
    lf = torch.empty((B, c.k_info), dtype=torch.float64, device="cuda")
    bits = c.decode_device(_dev(q), lfinal=lf, llr_step=step)
    return bits.cpu().numpy(), lf.cpu().numpy()


def test_decode_batch_matches_the_device_path(monkeypatch):
    c = _codec(48, "1/3")
    step = np.float32(0.3)
    chunk = 128
    x = _llrs(48, "1/3", chunk + 70)
    q = Q.quantize(x, step)
    for B in (1, 130):
        bits, lf = c.decode_batch(q[:B], return_lfinal=True, llr_step=step)
        want = _device_result(c, q[:B], step)
        assert bits.dtype == np.int32 and lf.dtype == np.float64
        assert np.array_equal(bits, want[0]) and np.array_equal(lf.view(np.uint64), want[1].view(np.uint64)), B
    # 70 codewords more than one host chunk: the second buffer and the chunk tail
    want = _device_result(c, q, step)
    monkeypatch.setenv("TDEC_HOST_CHUNK", str(chunk))
    bits, lf = c.decode_batch(q, return_lfinal=True, llr_step=step)
    f32 = c.decode_batch(Q.dequantize_i8(q, step))
    monkeypatch.delenv("TDEC_HOST_CHUNK")
    assert np.array_equal(bits, want[0]) and np.array_equal(lf.view(np.uint64), want[1].view(np.uint64))
    assert np.array_equal(f32, bits)               # and the float32 host path on the widened rows
    # float16 rows through the same door
    h = x.astype(np.float16)
    lfh = torch.empty((x.shape[0], c.k_info), dtype=torch.float64, device="cuda")
    wh = c.decode_device(_dev(h), lfinal=lfh)
    bh, lh = c.decode_batch(h, return_lfinal=True)
    assert np.array_equal(bh, wh.cpu().numpy()) and np.array_equal(lh.view(np.uint64), lfh.cpu().numpy().view(np.uint64))
    # decode() of one int8 vector is row 0
    assert np.array_equal(c.decode(q[0], llr_step=step), want[0][0])
    assert np.array_equal(c.decode(Q.quantize(x[0])), c.decode_batch(Q.quantize(x[:1]))[0])
    # a read-only and a non-contiguous array behave as their float32 counterparts: they decode
    ro = q[:65].copy()
    ro.setflags(write=False)
    wide = np.zeros((65, 2 * q.shape[1]), np.int8)
    wide[:, ::2] = q[:65]
    assert not wide[:, ::2].flags.c_contiguous
    for arr in (ro, wide[:, ::2]):
        assert np.array_equal(c.decode_batch(arr, llr_step=step), want[0][:65])
    fro = Q.dequantize_i8(ro, step)
    fro.setflags(write=False)
    assert np.array_equal(c.decode_batch(fro), want[0][:65])


# ---- 6. the pipeline's soft-bit link -------------------------------------------------------------------

def test_pipeline_link_is_its_three_calls():
    dev = torch.device("cuda", torch.cuda.current_device())
    c = _codec(48, "1/2")
    B, mod = 130, "QPSK"
    _, syms, n0 = W.make_symbols(c, B, mod, 4.0, 2025, dev, want_info=False)
    for llr, step in (("int8", None), ("int8", np.float32(0.3)), ("f16", None)):
        pipe = W.DevicePipeline(c, mod, B, dev, llr=llr, llr_step=step)
        got = _raw(pipe.run(syms, n0))
        flat = D.compute_llr_device(syms, mod, np.float64(n0), sign=-1).view(B, -1)
        if llr == "int8":
            q = D.quantize_llr_device(flat, Q.DEFAULT_STEP if step is None else step)
        else:
            q = flat.to(torch.float16)
        assert np.array_equal(got, _raw(c.decode_device(q, llr_step=step))), (llr, step)
    # llr="f32" is the pipeline as it was: the plane demapper, then the decoder
    plain = _raw(W.DevicePipeline(c, mod, B, dev).run(syms, n0))
    assert np.array_equal(_raw(W.DevicePipeline(c, mod, B, dev, llr="f32").run(syms, n0)), plain)
    planes = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device=dev)
    cons = D.constellation(mod)
    _, div32, nve = D.demap_mode(np.complex64, cons.dtype, np.float64(n0))
    c.demap_planes_device(syms, cons, 2, nve, planes, div_f32=div32)
    bits = torch.empty((B, c.k_info), dtype=torch.int32, device=dev)
    c.decode_planes_device(planes, B, bits)
    assert np.array_equal(_raw(bits), plain)
    assert plain.any() and not np.array_equal(got, np.zeros_like(got))


def test_harq_pipeline_link_combines_the_narrow_rows():
    dev = torch.device("cuda", torch.cuda.current_device())
    c = _codec(48, "1/2")
    B, mod, step = 65, "QPSK", np.float32(0.3)
    tx = [W.make_symbols(c, B, mod, 1.0, 7, dev, want_info=False, tx=t) for t in range(2)]
    for llr, st in (("int8", step), ("f16", None)):
        pipe = W.HarqPipeline([c], c, mod, B, dev, llr=llr, llr_step=st)
        planes = torch.empty(c.planes_bytes(B) // 4, dtype=torch.float32, device=dev)
        for t, (_, syms, n0) in enumerate(tx):
            got = _raw(pipe.receive(t, syms, n0))
            flat = D.compute_llr_device(syms, mod, np.float64(n0), sign=-1).view(B, -1)
            q = D.quantize_llr_device(flat, st) if llr == "int8" else flat.to(torch.float16)
            if t == 0:
                c.depuncture_device(q, planes, llr_step=st)
            else:
                c.depuncture_accumulate_device(q, planes, B, llr_step=st, f16=llr == "f16")
            bits = torch.empty((B, c.k_info), dtype=torch.int32, device=dev)
            c.decode_planes_device(planes, B, bits)
            assert np.array_equal(got, _raw(bits)), (llr, t)


# ---- 7. refusals -------------------------------------------------------------------------------------------

def test_abi_refusals():
    c = _codec(48, "1/2")
    L, h = N.lib(), c.handle.h
    walk = c.handle.llr_len
    c.reserve(65)
    q = torch.zeros((65, walk), dtype=torch.int8, device="cuda")
    x = torch.zeros(65 * walk, dtype=torch.float32, device="cuda")
    planes = torch.full((c.planes_bytes(65) // 4,), 7.0, dtype=torch.float32, device="cuda")
    bits = torch.full((65, c.k_info), 7, dtype=torch.int32, device="cuda")
    row = torch.zeros(65, dtype=torch.int32, device="cuda")
    qh, bh = np.zeros((65, walk), np.int8), np.full((65, c.k_info), 7, np.int32)
    P, I, E, S = N.ptr, N.LLRQ_KINDS["int8"], N.TDEC_EINVAL, N.TDEC_ESHORT
    F = N.LLRQ_KINDS["f16"]
    f = C.c_float
    bad_steps = (0.0, -0.25, float("inf"), float("nan"))
    cases = [(L.llrq_quantize_dev, (0, P(x), 0, -1, f(1), P(q), None, None), E),
             (L.llrq_quantize_dev, (0, None, 0, 8, f(1), P(q), None, None), E),
             (L.llrq_quantize_dev, (0, P(x), 0, 8, f(1), None, None, None), E),
             (L.llrq_depuncture_dev, (None, 65, P(q), I, f(1), walk, P(planes), None), E),
             (L.llrq_depuncture_dev, (h, -1, P(q), I, f(1), walk, P(planes), None), E),
             (L.llrq_depuncture_dev, (h, 65, None, I, f(1), walk, P(planes), None), E),
             (L.llrq_depuncture_dev, (h, 65, P(q), I, f(1), walk, None, None), E),
             (L.llrq_depuncture_dev, (h, 65, P(q), 2, f(1), walk, P(planes), None), E),
             (L.llrq_depuncture_dev, (h, 65, P(q), -1, f(1), walk, P(planes), None), E),
             (L.llrq_depuncture_dev, (h, 65, P(q), F, f(0.5), walk, P(planes), None), E),
             (L.llrq_depuncture_dev, (h, 65, P(q), I, f(1), walk - 1, P(planes), None), S),
             (L.llrq_depuncture_acc_dev, (None, 65, P(q), I, f(1), walk, 65, None, P(planes), None), E),
             (L.llrq_depuncture_acc_dev, (h, -1, P(q), I, f(1), walk, 65, None, P(planes), None), E),
             (L.llrq_depuncture_acc_dev, (h, 65, P(q), I, f(1), walk, -1, P(row), P(planes), None), E),
             (L.llrq_depuncture_acc_dev, (h, 65, None, I, f(1), walk, 65, None, P(planes), None), E),
             (L.llrq_depuncture_acc_dev, (h, 65, P(q), I, f(1), walk, 65, None, None, None), E),
             (L.llrq_depuncture_acc_dev, (h, 65, P(q), 7, f(1), walk, 65, None, P(planes), None), E),
             (L.llrq_depuncture_acc_dev, (h, 65, P(q), F, f(2), walk, 65, None, P(planes), None), E),
             (L.llrq_depuncture_acc_dev, (h, 65, P(q), I, f(1), walk, 64, None, P(planes), None), E),
             (L.llrq_depuncture_acc_dev, (h, 65, P(q), I, f(1), walk - 1, 65, None, P(planes), None), S),
             (L.llrq_decode_dev, (None, 0, 65, P(q), I, f(1), walk, P(bits), None, None, None), E),
             (L.llrq_decode_dev, (h, 4, 65, P(q), I, f(1), walk, P(bits), None, None, None), E),
             (L.llrq_decode_dev, (h, 0, -1, P(q), I, f(1), walk, P(bits), None, None, None), E),
             (L.llrq_decode_dev, (h, 0, 65, None, I, f(1), walk, P(bits), None, None, None), E),
             (L.llrq_decode_dev, (h, 0, 65, P(q), I, f(1), walk, None, None, None, None), E),
             (L.llrq_decode_dev, (h, 0, 65, P(q), 2, f(1), walk, P(bits), None, None, None), E),
             (L.llrq_decode_dev, (h, 0, 65, P(q), F, f(0.5), walk, P(bits), None, None, None), E),
             (L.llrq_decode_dev, (h, 0, 65, P(q), I, f(1), walk - 1, P(bits), None, None, None), S),
             (L.llrq_decode_batch, (None, 65, P(qh), I, f(1), walk, P(bh), None), E),
             (L.llrq_decode_batch, (h, -1, P(qh), I, f(1), walk, P(bh), None), E),
             (L.llrq_decode_batch, (h, 65, None, I, f(1), walk, P(bh), None), E),
             (L.llrq_decode_batch, (h, 65, P(qh), I, f(1), walk, None, None), E),
             (L.llrq_decode_batch, (h, 65, P(qh), 2, f(1), walk, P(bh), None), E),
             (L.llrq_decode_batch, (h, 65, P(qh), F, f(0.5), walk, P(bh), None), E),
             (L.llrq_decode_batch, (h, 65, P(qh), I, f(1), walk - 1, P(bh), None), S)]
    for s in bad_steps:
        cases += [(L.llrq_quantize_dev, (0, P(x), 0, 8, f(s), P(q), None, None), E),
                  (L.llrq_depuncture_dev, (h, 65, P(q), I, f(s), walk, P(planes), None), E),
                  (L.llrq_depuncture_acc_dev, (h, 65, P(q), I, f(s), walk, 65, None, P(planes), None), E),
                  (L.llrq_decode_dev, (h, 0, 65, P(q), I, f(s), walk, P(bits), None, None, None), E),
                  (L.llrq_decode_batch, (h, 65, P(qh), I, f(s), walk, P(bh), None), E)]
    for fn, args, want in cases:
        assert fn(*args) == want, (fn.__name__, args)
        assert L.tdec_last_error()
    # an empty batch is a no-op before the pointers are looked at
    assert L.llrq_quantize_dev(0, None, 0, 0, f(1), None, None, None) == 0
    assert L.llrq_depuncture_dev(h, 0, None, I, f(1), walk, None, None) == 0
    assert L.llrq_depuncture_acc_dev(h, 0, None, I, f(1), walk, 0, None, None, None) == 0
    assert L.llrq_decode_dev(h, 0, 0, None, I, f(1), walk, None, None, None, None) == 0
    assert L.llrq_decode_batch(h, 0, None, I, f(1), walk, None, None) == 0
    torch.cuda.synchronize()
    assert bool((planes == 7).all()) and bool((bits == 7).all()) and bool((q == 0).all()) and (bh == 7).all()


def test_python_refusals():
    dev = torch.device("cuda", torch.cuda.current_device())
    c = _codec(48, "1/2")
    walk = c.handle.llr_len
    planes = torch.full((c.planes_bytes(65) // 4,), 7.0, dtype=torch.float32, device="cuda")
    q = torch.zeros((65, walk), dtype=torch.int8, device="cuda")
    for dt in (torch.uint8, torch.int16, torch.bfloat16, torch.float64):
        t = torch.zeros((65, walk), dtype=dt, device="cuda")
        with pytest.raises(TypeError):
            c.decode_device(t)
        with pytest.raises(TypeError):
            c.depuncture_device(t, planes)
    for dt in (torch.uint8, torch.int16, torch.bfloat16):
        with pytest.raises(TypeError):
            c.depuncture_accumulate_device(torch.zeros((65, walk), dtype=dt, device="cuda"), planes, 65)
    h = q.to(torch.float16)
    f32 = q.to(torch.float32)
    for t in (h, f32):                                    # llr_step goes with int8 only
        with pytest.raises(TypeError):
            c.decode_device(t, llr_step=0.5)
        with pytest.raises(TypeError):
            c.depuncture_device(t, planes, llr_step=0.5)
        with pytest.raises(TypeError):
            c.depuncture_accumulate_device(t, planes, 65, llr_step=0.5, f16=True)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            c.decode_device(q, llr_step=bad)
        with pytest.raises(ValueError):
            c.depuncture_device(q, planes, llr_step=bad)
        with pytest.raises(ValueError):
            D.quantize_llr_device(f32, bad)
    with pytest.raises(IndexError):
        c.decode_device(q[:, :walk - 1])
    with pytest.raises(ValueError):
        c.depuncture_device(q[:, ::2], planes)             # rows not contiguous
    with pytest.raises(ValueError):
        c.depuncture_device(q, planes[:100])
    with pytest.raises(TypeError):
        D.quantize_llr_device(h)
    with pytest.raises(ValueError):
        D.quantize_llr_device(f32, out=torch.zeros((65, walk), dtype=torch.int16, device="cuda"))
    # numpy: uint8 and int16 are refused, llr_step needs int8, short rows are an IndexError
    qn = np.zeros((3, walk), np.int8)
    for dt in (np.uint8, np.int16):
        with pytest.raises(TypeError):
            c.decode_batch(qn.astype(dt))
        with pytest.raises(TypeError):
            c.decode(qn[0].astype(dt))
    with pytest.raises(TypeError):
        c.decode_batch(qn.astype(np.float16), llr_step=0.5)
    with pytest.raises(TypeError):
        c.decode_batch(qn.astype(np.float32), llr_step=0.5)
    with pytest.raises(ValueError):
        c.decode_batch(qn, llr_step=0.0)
    with pytest.raises(IndexError):
        c.decode_batch(qn[:, :walk - 1])
    with pytest.raises(ValueError):
        _codec(48, "1/2", early_stop=True).decode_batch(qn)
    # the pipelines: the plane demappers have no flat LLRs
    for kw in ({"fused": True}, {"overlap": True}):
        with pytest.raises(ValueError):
            W.DevicePipeline(c, "QPSK", 65, dev, llr="int8", **kw)
    with pytest.raises(ValueError):
        W.DevicePipeline(c, "QPSK", 65, dev, llr="int4")
    with pytest.raises(TypeError):
        W.DevicePipeline(c, "QPSK", 65, dev, llr="f16", llr_step=0.5)
    with pytest.raises(TypeError):
        W.HarqPipeline([c], c, "QPSK", 65, dev, llr="f32", llr_step=0.5)
    torch.cuda.synchronize()
    assert bool((planes == 7).all())
