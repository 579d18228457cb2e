"""Hybrid ARQ on the device: the soft-combining kernel against its
numpy restatement (tests/harq_ref.py), combined planes through every decoder against the
oracle, the generator's retransmissions against the entry points they must equal, and
workload.HarqPipeline against the reference chain.

The kernel comparisons are bit for bit with NaN at the same positions, over the whole plane
buffer read back through the documented tile layout plus guard words behind it.  Shapes are
the smallest that can go wrong: N = 48 and 212 (3 does not divide 212), every redundancy
version of rates 1/2, 2/3 and 3/4, 1 / 64 / 65 / 130 slots (tile boundary, ragged last tile),
f32 and f64 rows wider than the walk, row maps with holes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import codec_matrix as CM  # noqa: E402
import early_stop_ref as ES  # noqa: E402
import harq_ref as H  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import workload_ref as WR  # noqa: E402
from modulations_amd import _native as N  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd import workload as W  # noqa: E402

RATES = ("1/2", "2/3", "3/4")
VERSIONS = [(rate, rv) for rate in RATES for rv in range(T.PUNCTURE_PATTERNS[rate]["period"])]
SLOTS = (1, 64, 65, 130)
GUARD = 64
SPECIALS = np.array([-0.0, 0.0, 1e-45, -3e-39, np.inf, -np.inf, np.nan, 3e38], np.float32)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _codec(n, rate, rv=0, **kw):
    return M.DVBRCS2_Turbo(n, rate, interleaver="valid-perm", rv=rv, **kw)


def _sentinel(rng, size):
    """Plane values over a few decades with -0.0, denormals, +-inf and NaN sprinkled in."""
    x = (rng.standard_normal(size) * 10.0 ** rng.integers(-2, 3, size)).astype(np.float32)
    at = rng.random(size) < 0.08
    x[at] = SPECIALS[rng.integers(0, len(SPECIALS), int(at.sum()))]
    return x


def _row_maps(rng, n_slots):
    """(name, n_rows, row_of or None): the identity, a permutation, and a map with -1, with
    entries >= n_rows and with fewer rows than slots."""
    perm = rng.permutation(n_slots).astype(np.int32)
    n_rows = max(1, n_slots // 2)
    holes = rng.integers(-1, n_rows + 3, n_slots).astype(np.int32)
    holes[0] = -1
    if n_slots > 2:
        holes[1], holes[2] = n_rows, 0
    return [("null", n_slots, None), ("perm", n_slots, perm), ("holes", n_rows, holes)]


# ---- the kernel against the restatement ------------------------------------------------------

@pytest.mark.parametrize("rate,rv", VERSIONS)
@pytest.mark.parametrize("n", [48, 212])
def test_accumulate_matches_the_restatement(n, rate, rv):
    c = _codec(n, rate, rv)
    walk = H.walk(n, c.punct)[1]
    assert c.handle.llr_len == walk
    rng = np.random.default_rng([n, rv, RATES.index(rate)])
    for n_slots in SLOTS:
        tiles = -(-n_slots // 64)
        floats = tiles * H.tile_floats(n)
        assert c.planes_bytes(n_slots) == 4 * floats
        for f64 in (False, True):
            for name, n_rows, row_of in _row_maps(rng, n_slots):
                init = _sentinel(rng, floats + GUARD)
                llr = np.full((n_rows, walk + 7), np.nan, np.float64 if f64 else np.float32)   # stride > walk
                llr[:, :walk] = rng.standard_normal((n_rows, walk)) * 4.0
                sp = rng.random((n_rows, walk)) < 0.05
                llr[:, :walk][sp] = SPECIALS[rng.integers(0, len(SPECIALS), int(sp.sum()))]
                if f64:
                    llr[:, :walk] += 1e-9 * rng.standard_normal((n_rows, walk))               # not f32 values
                # the restatement over whole tiles: idle lanes of the last one are slots that take no row
                full = np.full(tiles * 64, -1, np.int64)
                full[:n_slots] = np.arange(n_slots) if row_of is None else row_of
                want6 = H.accumulate(H.from_tiles(init, tiles * 64, n), llr, n, c.punct, full)
                want = np.concatenate([H.to_tiles(want6), init[floats:]])
                planes = torch.from_numpy(init.copy()).cuda()
                d_llr = torch.from_numpy(llr).cuda()
                d_row = None if row_of is None else torch.from_numpy(row_of).cuda()
                c.depuncture_accumulate_device(d_llr, planes, n_slots, row_of=d_row)
                got = planes.cpu().numpy()
                assert H.same_bits(got, want), (n_slots, f64, name)
                if name == "holes":   # an untouched slot is bit-identical (NaN payloads too)
                    idle = np.nonzero((full < 0) | (full >= n_rows))[0]
                    g6, i6 = (H.from_tiles(a.view(np.float32), tiles * 64, n) for a in (got[:floats], init[:floats]))
                    assert np.array_equal(g6[idle].view(np.uint32), i6[idle].view(np.uint32))
                assert np.array_equal(got[floats:].view(np.uint32), init[floats:].view(np.uint32))   # guard words


def test_accumulate_special_values():
    """What the sentinel buffers must have exercised, on a hand-made case: inf + -inf = NaN as
    in the restatement, -0.0 kept where nothing is transmitted, a denormal sum kept."""
    n, c = 48, _codec(48, "3/4", 0)          # phase 0 sends W1 only; Y2 never
    src, walk = H.walk(n, c.punct)
    p6 = np.zeros((1, n, 6), np.float32)
    p6[0, 0] = [np.inf, 1e-45, -0.0, -0.0, -0.0, -0.0]
    llr = np.zeros((1, walk), np.float32)
    llr[0, src[0, 0]], llr[0, src[1, 0]], llr[0, src[2, 0]] = -np.inf, 1e-45, -0.0
    planes = torch.from_numpy(H.to_tiles(p6)).cuda()
    c.depuncture_accumulate_device(torch.from_numpy(llr).cuda(), planes, 1)
    got = H.from_tiles(planes.cpu().numpy(), 1, n)[0, 0]
    assert np.isnan(got[0]) and got[1] == np.float32(3e-45)
    assert np.array_equal(got[2:].view(np.uint32), np.float32([-0.0] * 4).view(np.uint32))   # -0 + -0, and untouched
    want = H.accumulate(p6.copy(), llr, n, c.punct)
    assert H.same_bits(got, want[0, 0])


# ---- combined planes through every decoder -----------------------------------------------------
DECODE_CASES = {"chase": (48, "1/2", [0, 0, 0]), "ir-3_4": (48, "3/4", [0, 1, 2, 3]), "ir-2_3": (212, "2/3", [0, 1, 2])}
NB = 65


@pytest.fixture(scope="module")
def combined():
    """Per case: the plane buffer after every transmission has been combined on the device
    (the first by tdec_depuncture_dev, the others by the kernel) and the restated rate-1/3
    vector, with the oracle's fixed decode and the restated early-stop rule on it.  Once."""
    out = {}
    for name, (n, rate, rvs) in DECODE_CASES.items():
        rng = np.random.default_rng([n, len(rvs)])
        info = rng.integers(0, 2, (NB, 2 * n)).astype(np.int32)
        codecs = [_codec(n, rate, rv) for rv in rvs]
        p6 = np.zeros((NB, n, 6), np.float32)
        planes = torch.zeros(codecs[0].planes_bytes(NB) // 4, dtype=torch.float32, device="cuda")
        for t, c in enumerate(codecs):
            coded = c.encode_batch(info)
            # low enough that no single transmission decodes every row, ramped over the rows
            llr = ES.bpsk_channel(coded, 2 * n, rng, np.linspace(-4.0, 1.0, NB))
            llr = np.ascontiguousarray(np.pad(llr, ((0, 0), (0, c.handle.llr_len - llr.shape[1]))))
            H.accumulate(p6, llr, n, c.punct)
            d = torch.from_numpy(llr).cuda()
            if t == 0:
                c.depuncture_device(d, planes)
            else:
                c.depuncture_accumulate_device(d, planes, NB)
        assert H.same_bits(H.from_tiles(planes.cpu().numpy(), NB, n), p6)
        third = T.PUNCTURE_PATTERNS["1/3"]
        perm, inv = CM.interleaver(n, "valid-perm")
        vec = H.llr6(p6)
        fixed = O.decode_batch(vec, n, 1, T.puncture_matrix(third), 8, perm, inv, CM.TAB, want_lfinal=True)
        es = ES.decode_early_stop_batch(vec, n, third, 8, perm, inv, CM.TAB, 0)
        out[name] = dict(n=n, planes=planes, info=info, fixed=fixed, es=es)
    return out


@pytest.mark.parametrize("case", list(DECODE_CASES))
def test_combined_planes_decode_as_the_oracle(combined, case):
    r = combined[case]
    n = r["n"]
    mother = _codec(n, "1/3")
    mother.reserve(NB)
    bits = torch.empty((NB, 2 * n), dtype=torch.int32, device="cuda")
    lf = torch.empty((NB, 2 * n), dtype=torch.float64, device="cuda")
    mother.decode_planes_device(r["planes"], NB, bits, lfinal=lf)
    assert np.array_equal(bits.cpu().numpy(), r["fixed"][0])
    assert np.array_equal(lf.cpu().numpy(), r["fixed"][1])
    assert (r["fixed"][0] != r["info"]).any(axis=1).sum() < NB           # combining decoded something
    counts = {}
    for dec in ("frame", "tile", "refill"):
        es = _codec(n, "1/3", early_stop=True, es_decoder=dec)
        es.reserve(NB)
        nit = torch.empty(NB, dtype=torch.int32, device="cuda")
        es.decode_planes_device(r["planes"], NB, bits, lfinal=lf, n_iter=nit)
        counts[dec] = nit.cpu().numpy()
        assert np.array_equal(bits.cpu().numpy(), r["es"][0]), dec
        assert np.array_equal(lf.cpu().numpy(), r["es"][1]), dec
        assert np.array_equal(counts[dec], r["es"][2]), dec
    assert np.array_equal(counts["frame"], counts["tile"]) and np.array_equal(counts["tile"], counts["refill"])
    assert len(set(counts["frame"].tolist())) >= 2


# ---- retransmissions of the generator ----------------------------------------------------------
GB, GSEED, GDB = 130, 4242, 3.0


def _tx_call(c, B, tx, cw0=0, fading=None, mod="QPSK", want_info=True):
    """harq_workload_tx_dev itself (make_symbols sends tx = 0 through the existing calls)."""
    bps, cons = D.MODULATIONS[mod]["bps"], D.constellation(mod)
    S = -(-c.handle.enc_len // bps)
    n0 = W.noise_n0(cons, c.k_info / c.n_coded, bps, GDB)
    table = np.ascontiguousarray(cons.astype(np.complex64)).view(np.float32)
    syms = torch.full((B, S), 7, dtype=torch.complex64, device="cuda")
    info = torch.full((B, c.k_info), 7, dtype=torch.uint8, device="cuda") if want_info else None
    coh = fading["coh"] if fading else 1
    h = torch.full((B, -(-S // coh)), 7, dtype=torch.complex64, device="cuda") if fading else None
    c.handle.call("harq_workload_tx_dev", B, tx, cw0, GSEED, N.ptr(table), len(cons), bps, float(np.sqrt(n0 / 2)),
                  int(fading is not None), fading["K"] if fading else 0.0, coh, N.ptr(syms), N.ptr(h), N.ptr(info),
                  c._stream(None))
    return info, syms, h


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_tx_identities():
    c = _codec(48, "1/2")
    info, syms, _ = W.make_symbols(c, GB, "QPSK", GDB, GSEED, "cuda")
    i0, s0, _ = _tx_call(c, GB, 0)
    assert _same(s0, syms) and _same(i0, info)                           # tx = 0: tdec_workload_dev
    fading = {"K": 1.5, "coh": 5}
    _, fs, _, fh = W.make_symbols(c, GB, "QPSK", GDB, GSEED, "cuda", fading=fading)
    i0, s0, h0 = _tx_call(c, GB, 0, fading=fading)
    assert _same(s0, fs) and _same(h0, fh) and _same(i0, info)           # tx = 0 faded: tdec_workload_fading_dev
    _, bs, _, bh = W.make_symbols(c, GB, "QPSK", GDB, GSEED, "cuda", fading={**fading, "branches": 8})
    for tx in (0, 1, 7):                                                 # tx = b faded: branch b
        ib, sb, hb = _tx_call(c, GB, tx, fading=fading)
        assert _same(sb, bs[:, tx]) and _same(hb, bh[:, tx]) and _same(ib, info), tx
        _, ms, _, mh = W.make_symbols(c, GB, "QPSK", GDB, GSEED, "cuda", fading=fading, tx=tx)
        assert _same(ms, sb) and _same(mh, hb)


def test_tx_noise_is_the_branch_stream():
    """Without fading: the same table points plus the noise of stream tx (restated in f64)."""
    c = _codec(48, "1/2")
    _, s0, _ = _tx_call(c, GB, 0)
    S = s0.shape[1]
    sigma = float(np.sqrt(W.noise_n0(D.constellation("QPSK"), c.k_info / c.n_coded, 2, GDB) / 2))
    cw = np.arange(GB)
    base = s0.cpu().numpy().astype(np.complex128) - WR.awgn(cw, S, GSEED, sigma)
    for tx in (1, 7):
        _, st, _ = _tx_call(c, GB, tx)
        assert not _same(st, s0)
        noise = st.cpu().numpy().astype(np.complex128) - base
        assert np.max(np.abs(noise - WR.awgn(cw, S, GSEED, sigma, branch=tx))) < 1e-5
        _, ms, _ = W.make_symbols(c, GB, "QPSK", GDB, GSEED, "cuda", tx=tx)
        assert _same(ms, st)


@pytest.mark.parametrize("fading", [None, {"K": 0.0, "coh": 7}])
def test_tx_split_invariance(fading):
    c = _codec(48, "3/4", rv=2)
    for tx in (0, 1, 7):
        whole = _tx_call(c, GB, tx, fading=fading)
        a, b = _tx_call(c, 60, tx, fading=fading), _tx_call(c, 70, tx, cw0=60, fading=fading)
        for w, x, y in zip(whole, a, b):
            assert (w is None and x is None) or _same(w, torch.cat([x, y])), tx


# ---- the pipeline against the reference chain --------------------------------------------------
# Eb/N0 (dB, per transmission) and generator seed chosen on the CPU from the reference chain below,
# fed with the restated generator (oracle/workload_ref.py: the device's info bits, its noise to
# about 1e-7): quarter-dB steps, the point where both shares asserted below have the most room.
# Chase (rate 1/2) at 2.0 dB: 18.5 % of the 130 rows ACK on the first transmission, 20.8 % need a
# third.  IR (rate 3/4) has a narrower window: at 1.25 dB, 16.9 % and 13.1 %.
PIPE_B, MAX_TX = 130, 4
PIPE_DB = {"chase": 2.0, "ir": 1.25}
PIPE_SEED = {"chase": 99, "ir": 109}


def _pipe_codecs(kind):
    if kind == "chase":
        c = _codec(48, "1/2")
        return [c], c
    return [_codec(48, "3/4", rv) for rv in range(4)], _codec(48, "1/3")


def reference_rounds(codecs, mother, syms, n0s, info):
    """The reference chain of a genie-aided HARQ run: per transmission oracle.demap (decoder sign)
    -> restated accumulate on the rows still wrong -> oracle.decode_batch of the mother code.
    syms[t]: complex64 [B, S_t]; returns per round (bits, active going in)."""
    n, B = mother.N, len(info)
    cons = D.constellation("QPSK")
    p6 = np.zeros((B, n, 6), np.float32)
    active = np.ones(B, bool)
    rounds = []
    for t, (y, n0) in enumerate(zip(syms, n0s)):
        c = codecs[t % len(codecs)]
        _, div_f32, nv = D.demap_mode(np.complex64, cons.dtype, np.float64(n0))
        llr = -O.demap(np.ascontiguousarray(y).reshape(-1), cons, 2, nv, div_f32).reshape(B, -1)
        H.accumulate(p6, llr, n, c.punct, np.where(active, np.arange(B), -1))
        bits = O.decode_batch(H.llr6(p6), n, 1, T.puncture_matrix(T.PUNCTURE_PATTERNS["1/3"]), mother.iterations,
                              mother.perm, mother.inv_perm, CM.TAB)
        rounds.append((bits, active.copy()))
        active = (bits != info).any(axis=1)
    return rounds


@pytest.mark.parametrize("kind", ["chase", "ir"])
def test_pipeline_matches_the_reference_chain(kind):
    codecs, mother = _pipe_codecs(kind)
    pipe = W.HarqPipeline(codecs, mother, "QPSK", PIPE_B, "cuda", max_tx=MAX_TX)
    info = W.info_bits(mother, PIPE_B, PIPE_SEED[kind], "cuda").cpu().numpy().astype(np.int32)
    tx = [W.make_symbols(pipe.codec(t), PIPE_B, "QPSK", PIPE_DB[kind], PIPE_SEED[kind], "cuda", want_info=False, tx=t)
          for t in range(MAX_TX)]
    ref = reference_rounds(codecs, mother, [s.cpu().numpy() for _, s, _ in tx], [n0 for _, _, n0 in tx], info)
    first_ack = 1.0 - ref[1][1].mean()            # rows not active going into round 1
    need_third = ref[2][1].mean()                 # rows active going into round 2
    print(kind, "Eb/N0", PIPE_DB[kind], "ACK on the first", first_ack, "need a third", need_third)
    assert first_ack >= 0.10 and need_third >= 0.10
    prev = None
    for t in range(MAX_TX):
        want, active = ref[t]
        act = None if t == 0 else torch.from_numpy(active if t % 2 else active.astype(np.int32)).cuda()   # bool / int32
        bits = pipe.receive(t, tx[t][1], tx[t][2], active=act).cpu().numpy()
        assert np.array_equal(bits, want), t
        if prev is not None:
            assert np.array_equal(bits[~active], prev[~active])          # inactive rows keep their bits
        prev = bits
    with pytest.raises(ValueError):
        pipe.receive(MAX_TX, tx[0][1], tx[0][2])
    with pytest.raises(ValueError):
        pipe.receive(0, tx[0][1], tx[0][2], active=torch.ones(PIPE_B, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError):
        pipe.receive(1, tx[1][1], tx[1][2], active=torch.ones(PIPE_B, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        pipe.receive(1, tx[1][1][:, :-1].contiguous(), tx[1][2])


def test_pipeline_takes_per_row_and_per_symbol_noise():
    """The tensor forms of noise_var, filled with one value, give the scalar's planes' bits."""
    codecs, mother = _pipe_codecs("ir")
    pipe = W.HarqPipeline(codecs, mother, "QPSK", 70, "cuda", max_tx=2)
    tx = [W.make_symbols(pipe.codec(t), 70, "QPSK", 0.5, 5, "cuda", want_info=False, tx=t) for t in range(2)]
    want = [pipe.receive(t, tx[t][1], tx[t][2]).clone() for t in range(2)]
    for shape in ((70,), None):
        for t in range(2):
            nv = torch.full(shape or tuple(tx[t][1].shape), tx[t][2], dtype=torch.float64, device="cuda")
            assert torch.equal(pipe.receive(t, tx[t][1], nv), want[t])


# ---- refusals ------------------------------------------------------------------------------------

def test_accumulate_refusals():
    c = _codec(48, "1/2")
    L, h, walk = N.lib(), c.handle.h, c.handle.llr_len
    planes = torch.full((c.planes_bytes(65) // 4,), 7, dtype=torch.float32, device="cuda")
    llr = torch.ones((65, walk), dtype=torch.float32, device="cuda")
    row = torch.zeros(65, dtype=torch.int32, device="cuda")
    p, q, r = planes.data_ptr(), llr.data_ptr(), row.data_ptr()
    E, S = N.TDEC_EINVAL, N.TDEC_ESHORT
    cases = [((None, 65, q, 0, walk, 65, None, p, None), E),            # null handle
             ((h, -1, q, 0, walk, 65, None, p, None), E),               # negative counts
             ((h, 65, q, 0, walk, -1, r, p, None), E),
             ((h, 0, None, 0, 0, 65, None, None, None), 0),             # empty: before the pointers and the stride
             ((h, 65, None, 0, walk, 65, None, p, None), E),            # null pointers with work to do
             ((h, 65, q, 0, walk, 65, None, None, None), E),
             ((h, 65, q, 0, walk - 1, 65, None, p, None), S),           # rows shorter than the walk
             ((h, 65, q, 1, walk - 1, 65, r, p, None), S),
             ((h, 65, q, 0, walk, 64, None, p, None), E)]               # null row_of, n_rows != n_slots
    for args, want in cases:
        assert L.harq_depuncture_acc_dev(*args) == want, args
        if want:
            assert L.tdec_last_error()
    torch.cuda.synchronize()
    assert bool((planes == 7).all())
    # the Python side
    with pytest.raises(ValueError):
        c.depuncture_accumulate_device(llr[:64], planes, 65)                                   # rows != slots
    with pytest.raises(ValueError):
        c.depuncture_accumulate_device(llr, planes, 65, row_of=row[:64])
    with pytest.raises(TypeError):
        c.depuncture_accumulate_device(llr, planes, 65, row_of=row.to(torch.int64))
    with pytest.raises(TypeError):
        c.depuncture_accumulate_device(llr.to(torch.float16), planes, 65)
    with pytest.raises(IndexError):
        c.depuncture_accumulate_device(llr[:, :walk - 1], planes, 65)
    with pytest.raises(ValueError):
        c.depuncture_accumulate_device(llr, planes[:100], 65)
    with pytest.raises(ValueError):
        c.depuncture_accumulate_device(llr[:, ::2], planes, 65)                                # rows not contiguous
    torch.cuda.synchronize()
    assert bool((planes == 7).all())


def test_tx_refusals():
    c = _codec(48, "1/2")
    L, h = N.lib(), c.handle.h
    table = np.ascontiguousarray(D.constellation("QPSK").astype(np.complex64)).view(np.float32)
    S = c.n_coded // 2
    syms = torch.full((4, S), 7, dtype=torch.complex64, device="cuda")
    gains = torch.full((4, S), 7, dtype=torch.complex64, device="cuda")
    t, y, g = N.ptr(table), syms.data_ptr(), gains.data_ptr()

    def call(hh=h, B=4, tx=1, cw0=0, cons=t, M_=4, bps=2, sigma=0.5, fading=0, k=0.0, coh=1, sy=y, gh=g):
        return L.harq_workload_tx_dev(hh, B, tx, cw0, 1, cons, M_, bps, sigma, fading, k, coh, sy, gh, None, None)
    E = N.TDEC_EINVAL
    assert call(hh=None) == E and call(B=-1) == E and call(cw0=-1) == E
    assert call(tx=-1) == E and call(tx=65536) == E
    assert call(B=0, cons=None, sy=None) == 0
    assert call(cons=None) == E and call(sy=None) == E and call(M_=8) == E and call(sigma=-1.0) == E
    assert call(fading=1, gh=None) == E and call(fading=1, coh=0) == E and call(fading=1, k=-1.0) == E
    torch.cuda.synchronize()
    assert bool((syms == 7).all()) and bool((gains == 7).all())
    assert call(fading=0, gh=None, coh=0, k=-1.0) == 0                   # not looked at without fading
    syms.fill_(7)
    assert call(tx=65535, fading=1) == 0
    torch.cuda.synchronize()
    assert not bool((syms == 7).any())
    with pytest.raises(ValueError):
        W.make_symbols(c, 4, "QPSK", 3.0, 1, "cuda", tx=65536)
    with pytest.raises(ValueError):
        W.make_symbols(c, 4, "QPSK", 3.0, 1, "cuda", tx=-1)
    with pytest.raises(ValueError):
        W.make_symbols(c, 4, "QPSK", 3.0, 1, "cuda", tx=1, fading={"K": 0.0, "coh": 1, "branches": 2})
    with pytest.raises(ValueError):
        W.make_symbols(c, 4, "QPSK", 3.0, 1, "cuda", tx=1, fading={"K": 0.0, "coh": 1}, pilots=D.PilotLayout(2, 12))
