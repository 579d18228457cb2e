"""The frame check on the device (include/crc.h) against its bitwise
restatement (tests/crc_ref.py): verify (ok and remainder), attach (bytes written and bytes
left alone), the generator fed with the caller's info bits against the entry points it must
equal, and every refusal.  All comparisons are exact.

Shapes are the smallest that can go wrong.  Row lengths, both kinds: r + 8 (one payload byte),
96 (less than one sweep of the wave), 424 (a partly filled last sweep), 1504, 1696, 2048 (the
longest).  Batches 1 / 63 / 64 / 65 / 130, and STRIDE_B rows, with which every block of the
launch's grid takes a second grid-stride trip.  A base pointer one element past an aligned one
takes the element loads."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import crc_ref as R  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import crc as CRC  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

KINDS = ("crc16", "crc32")
BATCHES = (1, 63, 64, 65, 130)
# the launch covers GRID_ROWS rows per trip of its grid (CRC_MAX_BLOCKS blocks of CRC_ROWS_PER_BLOCK
# rows): with twice that and a few more, every block makes a second trip and the first a third
STRIDE_B = 2 * CRC.GRID_ROWS + 3
GUARD = 64


def lengths(kind):
    return (R.KINDS[kind][0] + 8, 96, 424, 1504, 1696, 2048)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rows(rng, kind, B, L):
    """int32 [B][L]: random rows, every third one valid, then (over some of those) all-zero, all-one
    and rows whose elements are 2, 3 and -1 where B has room for them."""
    rows = rng.integers(0, 2, (B, L)).astype(np.int32)
    rows[::3] = R.attach(rows[::3], kind)
    for i, fill in zip(range(1, B, max(1, B // 6)), (0, 1, 2, 3, -1)):
        rows[i] = fill
    if B > 8:
        rows[8] = R.attach(rows[8], kind)[0] + 2 * rng.integers(-3, 4, L)    # valid, with the other bits set
    return rows


def _device_rows(rows, dtype, offset):
    """The rows on the device behind `offset` elements of padding: offset 0 is torch's aligned
    allocation, offset 1 one element past it."""
    flat = torch.zeros(rows.size + offset, dtype=dtype, device="cuda")
    view = flat[offset:].view(rows.shape)
    view.copy_(torch.from_numpy(rows).to(dtype))
    assert view.data_ptr() % 16 == (offset * view.element_size()) % 16
    return view


def _check(rows, kind, dtype, offset=0):
    d = _device_rows(rows, dtype, offset)
    rem = torch.full((len(rows),), 7, dtype=torch.int32, device="cuda")
    ok = CRC.check_device(d, kind, rem=rem)
    return ok.cpu().numpy(), rem.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", KINDS)
def test_verify_matches_the_restatement(kind):
    rng = np.random.default_rng([1, R.KINDS[kind][0]])
    for L in lengths(kind):
        for B in BATCHES:
            rows = _rows(rng, kind, B, L)
            want = R.remainder(rows, kind)
            assert want[0] == 0 and (B < 9 or want[8] == 0) and (B < 3 or (want != 0).any())
            for dtype, offset in ((torch.int32, 0), (torch.int32, 1), (torch.uint8, 0), (torch.uint8, 1)):
                ok, rem = _check(rows & 1 if dtype == torch.uint8 else rows, kind, dtype, offset)
                assert np.array_equal(rem, want), (L, B, dtype, offset)
                assert np.array_equal(ok, (want == 0).astype(np.int32)), (L, B, dtype, offset)


@pytest.mark.parametrize("kind", KINDS)
def test_verify_grid_stride(kind):
    rng = np.random.default_rng([2, R.KINDS[kind][0]])
    rows = rng.integers(0, 2, (STRIDE_B, 96)).astype(np.int32)
    rows[::2] = R.attach(rows[::2], kind)
    want = R.remainder(rows, kind)
    for dtype in (torch.int32, torch.uint8):
        ok, rem = _check(rows, kind, dtype)
        assert np.array_equal(rem, want) and np.array_equal(ok, (want == 0).astype(np.int32)), dtype
    d = _device_rows(rows, torch.int32, 0)
    ok = torch.full((STRIDE_B,), 7, dtype=torch.int32, device="cuda")
    CRC.check_device(d, kind, ok=ok)                                          # without the remainder
    assert np.array_equal(ok.cpu().numpy(), (want == 0).astype(np.int32))


@pytest.mark.parametrize("L", [96, 424])
@pytest.mark.parametrize("kind", KINDS)
def test_designed_rows(kind, L):
    r = R.KINDS[kind][0]
    rng = np.random.default_rng([3, r, L])
    valid = R.attach(rng.integers(0, 2, (1, L)).astype(np.int32), kind)[0]
    assert R.remainder(valid, kind)[0] == 0
    # every single-bit flip, one row per position
    flips = np.tile(valid, (L, 1))
    flips[np.arange(L), np.arange(L)] ^= 1
    want = R.remainder(flips, kind)
    assert (want != 0).all() and len(set(want.tolist())) == L
    ok, rem = _check(flips, kind, torch.int32)
    assert np.array_equal(rem, want) and not ok.any()
    # bursts of every length <= r (both ends set; the interior random, and all set) at the first, a middle
    # and the last offset
    bursts = []
    for n in range(1, r + 1):
        for inner in (rng.integers(0, 2, max(0, n - 2)), np.ones(max(0, n - 2), np.int64)):
            pat = np.ones(n, np.int32)
            pat[1:n - 1] = inner[:max(0, n - 2)]
            for at in (0, (L - n) // 2, L - n):
                row = valid.copy()
                row[at:at + n] ^= pat
                bursts.append(row)
    bursts = np.stack(bursts)
    want = R.remainder(bursts, kind)
    assert (want != 0).all()
    ok, rem = _check(bursts, kind, torch.int32)
    assert np.array_equal(rem, want) and not ok.any()
    ok, rem = _check(bursts, kind, torch.uint8)
    assert np.array_equal(rem, want) and not ok.any()
    # a multiple of g(x) added to a valid row is a valid row: the check is polynomial arithmetic
    g = R.g_bits(kind).astype(np.int32)
    shifted = []
    for at in (0, 1, L - r - 1):
        row = valid.copy()
        row[at:at + r + 1] ^= g
        assert (row != valid).any()
        shifted.append(row)
    shifted = np.stack(shifted)
    assert (R.remainder(shifted, kind) == 0).all()
    ok, rem = _check(shifted, kind, torch.int32)
    assert ok.all() and not rem.any()


@pytest.mark.parametrize("kind", KINDS)
def test_attach_writes_the_check_field_only(kind):
    r = R.KINDS[kind][0]
    rng = np.random.default_rng([4, r])
    for L in lengths(kind):
        for B in BATCHES:
            rows = rng.integers(0, 2, (B, L)).astype(np.uint8)
            rows[:, -r:] = 7                                                   # what attach must overwrite
            want = R.attach(rows, kind)
            for offset in (0, 1):
                flat = torch.full((offset + B * L + GUARD,), 9, dtype=torch.uint8, device="cuda")
                view = flat[offset:offset + B * L].view(B, L)
                view.copy_(torch.from_numpy(rows))
                assert CRC.attach_device(view, kind) is view
                got = flat.cpu().numpy()
                assert (got[:offset] == 9).all() and (got[offset + B * L:] == 9).all(), (L, B, offset)   # guards
                got = got[offset:offset + B * L].reshape(B, L)
                assert np.array_equal(got[:, :-r], rows[:, :-r]), (L, B, offset)                         # payload
                assert np.array_equal(got, want), (L, B, offset)
                ok = CRC.check_device(view, kind)                              # attach then verify passes
                assert bool(ok.all())
                assert bool(CRC.check_device(view.to(torch.int32), kind).all())


def test_attach_grid_stride():
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 2, (STRIDE_B, 96)).astype(np.uint8)
    d = torch.from_numpy(rows).cuda()
    CRC.attach_device(d, "crc32")
    assert np.array_equal(d.cpu().numpy(), R.attach(rows, "crc32"))
    assert bool(CRC.check_device(d, "crc32").all())


# ---- the generator with the caller's info bits ---------------------------------------------------
GSEED, GDB = 4242, 3.0


def _codec(n, rate):
    return M.DVBRCS2_Turbo(n, rate, interleaver="valid-perm")


def _args(c, mod, sigma=None):
    bps, cons = D.MODULATIONS[mod]["bps"], D.constellation(mod)
    n0 = W.noise_n0(cons, c.k_info / c.n_coded, bps, GDB)
    table = np.ascontiguousarray(cons.astype(np.complex64)).view(np.float32)
    return table, len(cons), bps, float(np.sqrt(n0 / 2)) if sigma is None else sigma, -(-c.handle.enc_len // bps)


def _tx(c, name, B, tx, mod, fading, bits=None, sigma=None, cw0=0):
    """harq_workload_tx_dev, or crc_workload_tx_dev with `bits`."""
    table, m, bps, sg, S = _args(c, mod, sigma)
    coh = fading["coh"] if fading else 1
    syms = torch.full((B, S), 7, dtype=torch.complex64, device="cuda")
    h = torch.full((B, -(-S // coh)), 7, dtype=torch.complex64, device="cuda") if fading else None
    head = (B, tx, cw0, GSEED, N.ptr(table), m, bps, sg, int(fading is not None), fading["K"] if fading else 0.0, coh)
    tail = (N.ptr(syms), N.ptr(h), None) if name == "harq_workload_tx_dev" else (N.ptr(bits), N.ptr(syms), N.ptr(h))
    c.handle.call(name, *head, *tail, c._stream(None))
    return syms, h


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("n,rate,mod", [(48, "1/2", "QPSK"), (212, "2/3", "16QAM")])
def test_generator_identity(n, rate, mod):
    c, B = _codec(n, rate), 130
    info = W.info_bits(c, B, GSEED, "cuda")
    for fading in (None, {"K": 1.5, "coh": 5}):
        for tx in (0, 3):
            want = _tx(c, "harq_workload_tx_dev", B, tx, mod, fading)
            got = _tx(c, "crc_workload_tx_dev", B, tx, mod, fading, bits=info)
            assert _same(got[0], want[0]), (tx, fading)
            assert (fading is None and got[1] is None) or _same(got[1], want[1]), (tx, fading)
    # split invariance with a batch offset: codeword cw0 + c takes row c of the bits
    whole = _tx(c, "crc_workload_tx_dev", B, 3, mod, None, bits=info)[0]
    tail = _tx(c, "crc_workload_tx_dev", B - 60, 3, mod, None, bits=info[60:].contiguous(), cw0=60)[0]
    assert _same(whole[60:], tail)


@pytest.mark.parametrize("n,rate,mod", [(48, "1/2", "QPSK"), (212, "2/3", "16QAM")])
@pytest.mark.parametrize("kind", KINDS)
def test_attached_bits_are_what_is_encoded(n, rate, mod, kind):
    """Without noise a symbol is its table point: the labels read back are the coded stream, which
    must be encode_device of the info bits with the check field."""
    c, B = _codec(n, rate), 65
    r = R.KINDS[kind][0]
    plain = W.info_bits(c, B, GSEED, "cuda")
    info, syms, _ = W.make_symbols(c, B, mod, GDB, GSEED, "cuda", crc=kind)
    assert np.array_equal(info.cpu().numpy(), R.attach(plain.cpu().numpy(), kind))
    assert _same(info[:, :-r], plain[:, :-r]) and bool(CRC.check_device(info, kind).all())
    clean, _ = _tx(c, "crc_workload_tx_dev", B, 0, mod, None, bits=info, sigma=0.0)
    cons = D.constellation(mod).astype(np.complex64)
    bps = D.MODULATIONS[mod]["bps"]
    y = clean.cpu().numpy()
    labels = np.argmax(y[:, :, None] == cons[None, None, :], axis=2)
    assert (cons[labels] == y).all()
    stream = ((labels[:, :, None] >> np.arange(bps - 1, -1, -1)) & 1).reshape(B, -1).astype(np.uint8)
    coded = c.encode_device(info).cpu().numpy()
    assert np.array_equal(stream[:, :coded.shape[1]], coded) and not stream[:, coded.shape[1]:].any()
    # and the noisy symbols are those points plus the noise of the plain generator
    _, psyms, _ = W.make_symbols(c, B, mod, GDB, GSEED, "cuda")
    pclean, _ = _tx(c, "crc_workload_tx_dev", B, 0, mod, None, bits=plain, sigma=0.0)
    same_point = (clean == pclean)
    assert bool(same_point.any()) and not bool(same_point.all())
    assert torch.equal(syms[same_point], psyms[same_point])


def test_make_symbols_crc_with_tx_and_fading():
    c, B = _codec(48, "1/2"), 70
    fading = {"K": 0.0, "coh": 7}
    info, syms, n0, gains = W.make_symbols(c, B, "QPSK", GDB, GSEED, "cuda", fading=fading, tx=2, crc="crc16")
    want = _tx(c, "crc_workload_tx_dev", B, 2, "QPSK", fading, bits=info)
    assert _same(syms, want[0]) and _same(gains, want[1])
    _, _, n0p, plain_gains = W.make_symbols(c, B, "QPSK", GDB, GSEED, "cuda", fading=fading, tx=2)
    assert n0 == n0p and _same(gains, plain_gains)                            # the check field is not charged
    none, s2, _ = W.make_symbols(c, B, "QPSK", GDB, GSEED, "cuda", tx=2, crc="crc16", want_info=False)
    assert none is None and _same(s2, _tx(c, "crc_workload_tx_dev", B, 2, "QPSK", None, bits=info)[0])
    with pytest.raises(ValueError):
        W.make_symbols(c, B, "QPSK", GDB, GSEED, "cuda", fading={**fading, "branches": 2}, crc="crc16")
    with pytest.raises(ValueError):
        W.make_symbols(c, B, "QPSK", GDB, GSEED, "cuda", fading=fading, pilots=D.PilotLayout(2, 12), crc="crc16")
    with pytest.raises(ValueError):
        W.make_symbols(c, B, "QPSK", GDB, GSEED, "cuda", crc="crc8")


# ---- refusals --------------------------------------------------------------------------------------

def test_crc_refusals():
    L = N.lib()
    E = N.TDEC_EINVAL
    rows = torch.full((4, 96), 7, dtype=torch.uint8, device="cuda")
    bits = torch.zeros((4, 96), dtype=torch.int32, device="cuda")
    ok = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    p, q, o = rows.data_ptr(), bits.data_ptr(), ok.data_ptr()

    def attach(kind=16, B=4, row_bits=96, ptr=p):
        return L.crc_attach_dev(0, kind, B, row_bits, ptr, None)

    def check(kind=16, B=4, row_bits=96, ptr=q, okp=o, fn=L.crc_check_dev):
        return fn(0, kind, B, row_bits, ptr, okp, None, None)
    for call in (attach, check, lambda **kw: check(fn=L.crc_check_u8_dev, **kw)):
        assert call(kind=8) == E and call(kind=0) == E and call(kind=24) == E          # unknown kind
        assert call(row_bits=100) == E and call(row_bits=92) == E                      # not whole bytes
        assert call(row_bits=16) == E and call(row_bits=8) == E                        # row_bits <= r
        assert call(kind=32, row_bits=32) == E
        assert call(row_bits=2056) == E and call(row_bits=4096) == E                   # too long
        assert call(B=-1) == E
        assert call(ptr=None) == E                                                     # null with work to do
        assert L.tdec_last_error()
        assert call(B=0, ptr=None) == 0                                                # empty: before the pointers
    assert check(okp=None) == E
    assert check(B=0, ptr=None, okp=None) == 0
    torch.cuda.synchronize()
    assert bool((rows == 7).all()) and bool((ok == 7).all())
    assert attach(row_bits=24) == 0 and attach(kind=32, row_bits=40) == 0 and attach(row_bits=2048, B=0) == 0
    # the generator
    c = _codec(48, "1/2")
    h = c.handle.h
    table, m, bps, sg, S = _args(c, "QPSK")
    info = W.info_bits(c, 4, 1, "cuda")
    syms = torch.full((4, S), 7, dtype=torch.complex64, device="cuda")
    gains = torch.full((4, S), 7, dtype=torch.complex64, device="cuda")

    def tx(hh=h, B=4, t=1, cw0=0, cons=N.ptr(table), M_=m, sigma=sg, fading=0, k=0.0, coh=1, b=info.data_ptr(),
           sy=syms.data_ptr(), gh=gains.data_ptr()):
        return L.crc_workload_tx_dev(hh, B, t, cw0, 1, cons, M_, bps, sigma, fading, k, coh, b, sy, gh, None)
    assert tx(hh=None) == E and tx(B=-1) == E and tx(cw0=-1) == E and tx(t=-1) == E and tx(t=65536) == E
    assert tx(b=None) == E                                                             # null d_bits_in
    assert tx(cons=None) == E and tx(sy=None) == E and tx(M_=8) == E and tx(sigma=-1.0) == E
    assert tx(fading=1, gh=None) == E and tx(fading=1, coh=0) == E and tx(fading=1, k=-1.0) == E
    assert tx(B=0, b=None, cons=None, sy=None) == 0
    torch.cuda.synchronize()
    assert bool((syms == 7).all()) and bool((gains == 7).all())
    assert tx(fading=0, gh=None, coh=0, k=-1.0) == 0                                   # not looked at without fading
    torch.cuda.synchronize()
    assert not bool((syms == 7).any())
    # the Python side
    with pytest.raises(ValueError):
        CRC.check_device(bits, "crc24")
    with pytest.raises(TypeError):
        CRC.check_device(bits.to(torch.int64), "crc16")
    with pytest.raises(TypeError):
        CRC.attach_device(bits, "crc16")
    with pytest.raises(ValueError):
        CRC.check_device(bits[:, ::2], "crc16")
    with pytest.raises(ValueError):
        CRC.check_device(bits, "crc16", ok=ok[:3])
    with pytest.raises(ValueError):
        CRC.check_device(bits, "crc16", rem=ok.to(torch.int64))
    with pytest.raises(ValueError):
        CRC.check_device(torch.zeros((4, 16), dtype=torch.int32, device="cuda"), "crc16")   # row_bits <= r
