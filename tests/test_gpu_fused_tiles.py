"""The fused demap + decode kernel (k_turbo_decode_syms, all four instantiations) with several
tiles per wave.

From a wave's second tile on, the fused prologue (DemapPro, tdec_demap_kernels.hip) matters in
ways its first tile cannot show: the next tile is demapped in 2 x iterations pieces between the
SISOs of the current one, into the other of the wave's two plane buffers (buf ^= 1); publish()
invalidates L1 before a reused buffer is read (from the third tile); lanes past B and LLRs past
n_avail must be written as 0, not as what the never-cleared LDS chunk or the reused buffer held
from the tile before.  TDEC_TILE_WAVES (read per call, tdec_api.hip tile_queue()) caps the
persistent waves of the launch, so the ten tiles of B = 581 come from the tile queue (cap "1",
"2"), by static striding at 3 to 4 tiles per wave (cap "3"), or one per wave (unset).

Reference, as in test_gpu_fused.py: the two-launch path (demap_planes_device, then
decode_planes_device) with the cap unset, which the other tests pin to the oracle; bits and
L_final must be equal (IEEE ==; NaN == NaN only in the cases with NaN symbols).  Each case's
reference is computed once and carries an oracle spot check of six rows: the first and last row
of the first, a middle and the last tile.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("trans_tables")]

from oracle import oracle as O  # noqa: E402
from modulations_amd import _native as NT  # noqa: E402
from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd import tables as T  # noqa: E402
from modulations_amd.workload import DevicePipeline, make_symbols  # noqa: E402
from test_gpu_demap_split import _adversarial  # noqa: E402

CAP = "TDEC_TILE_WAVES"
B = 581                          # nine full tiles and one of 5 rows
SPOT = [0, 63, 256, 319, 576, 580]
CAPS = ["1", "2", "3", None]
CAP_IDS = ["cap1", "cap2", "cap3", "unset"]
# the instantiations of fused_kernel() (tdec_demap_api.hip): modulation -> decoder algorithm
KERNELS = {"16QAM": "max-log", "256QAM": "max-log", "QPSK": "max-log", "8PSK": "log-map"}
TABLE = {"16QAM": np.complex64, "256QAM": np.complex64, "QPSK": np.complex128, "8PSK": np.complex64}


class Case:
    """One fused configuration.  ds: symbols per row relative to ceil(n_coded / bps).
    adv: None (the workload generator's symbols at 2 dB) or the noise variance of adversarial
    symbols (_adversarial; 1e5 with the symbols scaled by 300, as test_gpu_demap_split does)."""

    def __init__(self, mod, n, rate, iters=8, ds=0, adv=None):
        self.mod, self.n, self.rate, self.iters, self.ds, self.adv = mod, n, rate, iters, ds, adv
        self.algo = KERNELS[mod]
        nv = "" if adv is None else ("-adv-f32" if isinstance(adv, np.float32) else f"-adv-{adv:g}")
        self.id = f"{mod}-{n}-{rate.replace('/', '_')}" + (f"-it{iters}" if iters != 8 else "") + \
            (f"-S{ds:+d}" if ds else "") + nv


CASES = (
    # every instantiation, N = 48 (6 chunks of 8 couples: fewer than the 16 pieces) and N = 212
    [Case(m, 48, "1/3") for m in KERNELS] + [Case(m, 212, "1/2") for m in KERNELS] +
    # rate 3/4: symbols straddle the chunks, W2 once a period, Y2 never (src = -1 on whole components)
    [Case("8PSK", 64, "3/4"), Case("256QAM", 64, "3/4"),
     # rate 2/3 at N = 212: n_coded is shorter than the de-puncture walk
     Case("16QAM", 212, "2/3")] +
    # 2 and 4 pieces for N = 48's 6 chunks (16 pieces: the 8-iteration cases above)
    [Case(m, 48, "1/3", iters=i) for m in ("16QAM", "8PSK") for i in (1, 2)] +
    # fewer symbols than the code needs (LLRs past n_avail are 0 in every tile) and a surplus (ignored)
    [Case("16QAM", 48, "1/3", ds=-3), Case("16QAM", 48, "1/3", ds=+2), Case("256QAM", 212, "1/2", ds=-3),
     Case("8PSK", 64, "3/4", ds=-3), Case("QPSK", 48, "1/3", ds=+2)] +
    # symbols the fast searches decline; the unscaled divisions' range, outside it, the f32 quotient
    [Case(m, n, r, adv=nv) for m, n, r in (("16QAM", 212, "1/2"), ("256QAM", 48, "1/3"))
     for nv in (0.04, 1e5, np.float32(0.037))])
CASE_IDS = [c.id for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv(CAP, raising=False)
    else:
        monkeypatch.setenv(CAP, cap)


def _poison(s):
    """Symbols whose LLRs are not finite: NaN, inf, or so large that |z|^2 overflows float32."""
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(s.real) & np.isfinite(s.imag) & (np.abs(s.real) < 1e18) & (np.abs(s.imag) < 1e18))


def _adversarial_rows(case, cons, bps, S):
    """_adversarial spreads its NaN / inf / overflowing tenth over every row; rows 0, 3, 6, ... of the
    batch get bisector ties (finite, still declined by the fast searches) there instead, so that every
    tile holds rows that must stay finite beside rows that must not."""
    rng = np.random.default_rng([case.n, bps, int(float(case.adv) * 1000) % 9973])
    s = _adversarial(cons, rng, (B, S))
    lv = np.unique(cons.real.astype(np.float64))
    mids = (lv[:-1] + lv[1:]) / 2
    bad = _poison(s)
    bad[np.arange(B) % 3 != 0] = False
    s[bad] = (rng.choice(mids, int(bad.sum())) + 1j * rng.choice(lv, int(bad.sum()))).astype(np.complex64)
    if float(case.adv) > 1:   # outside the unscaled divisions' range, as test_gpu_demap_split scales them
        with np.errstate(over="ignore", invalid="ignore"):
            s = (s * 300).astype(np.complex64)
    return s


def _symbols(case, codec, cons, bps):
    S0 = -(-codec.n_coded // bps)
    if case.adv is not None:
        # a float64 noise variance divides in f64, a float32 one in f32 (numpy's rule, demap_mode)
        nv = case.adv if isinstance(case.adv, np.float32) else np.float64(case.adv)
        return torch.from_numpy(_adversarial_rows(case, cons, bps, S0)).cuda(), nv
    _, syms, n0 = make_symbols(codec, B, case.mod, 2.0, 1000 + case.n, "cuda", want_info=False)
    # the generator sends encode()'s own length, which at rate 2/3 with 3 not dividing N is longer than
    # n_coded; the receiver's count is ceil(n_coded / bps), as in the reference's chain
    assert syms.shape[0] == B and S0 <= syms.shape[1] <= S0 + 1
    syms = syms[:, :S0 + min(case.ds, 0)].contiguous()
    if case.ds > 0:   # the surplus is NaN: were it read, it would poison its row
        syms = torch.cat([syms, torch.full((B, case.ds), np.nan, dtype=syms.dtype, device="cuda")], 1).contiguous()
    return syms, np.float64(n0)


def _oracle_rows(case, codec, cons, bps, syms, nve, div32):
    """The host chain on a few rows: compute_llr (decoder sign; a NaN symbol gives NaN LLRs), f32,
    truncated / zero-padded to the de-puncture walk, the oracle's decode."""
    L = codec.handle.llr_len
    llr = np.zeros((len(syms), L), np.float32)
    for i, r in enumerate(syms):
        v = np.full(len(r) * bps, np.nan)
        fin = ~np.isnan(r)
        v.reshape(-1, bps)[fin] = (-O.demap(r[fin], cons, bps, nve, div_f32=div32)).reshape(-1, bps)
        m = min(L, len(v))
        llr[i, :m] = v[:m]
    t, _ = O.trellis()
    return O.decode_batch(llr, case.n, codec.punct["period"], T.puncture_matrix(codec.punct), case.iters, codec.perm,
                          codec.inv_perm, t, algo=codec.algo, want_lfinal=True)


@pytest.fixture(scope="module")
def prepared():
    """Per case, once: the codec (reserved for both paths), the symbols, the two-launch reference
    with the cap unset, and its oracle spot check."""
    cache = {}

    def get(case, monkeypatch):
        if case.id not in cache:
            monkeypatch.delenv(CAP, raising=False)
            codec = M.DVBRCS2_Turbo(case.n, case.rate, case.iters, algo=case.algo, inv_perm="stable")
            bps = D.MODULATIONS[case.mod]["bps"]
            cons = D.constellation(case.mod)
            assert cons.dtype == TABLE[case.mod] and codec.fused_available(cons, bps)
            syms, nv = _symbols(case, codec, cons, bps)
            _, div32, nve = D.demap_mode(np.complex64, cons.dtype, nv)
            assert div32 == isinstance(nv, np.float32)
            pipe = DevicePipeline(codec, case.mod, B, "cuda", fused=False)
            bits = torch.full((B, codec.k_info), 7, dtype=torch.int32, device="cuda")
            lf = torch.full((B, codec.k_info), np.nan, dtype=torch.float64, device="cuda")
            codec.demap_planes_device(syms, cons, bps, nve, pipe.planes, div_f32=div32)
            codec.decode_planes_device(pipe.planes, B, bits, lfinal=lf)
            torch.cuda.synchronize()
            rb, rl = _oracle_rows(case, codec, cons, bps, syms[SPOT].cpu().numpy(), nve, div32)
            assert np.array_equal(bits[SPOT].cpu().numpy(), rb)
            np.testing.assert_array_equal(lf[SPOT].cpu().numpy(), rl)
            codec.reserve_fused(B)
            cache[case.id] = codec, cons, bps, syms, nve, div32, bits, lf
        return cache[case.id]

    yield get
    cache.clear()


def _fused(codec, cons, bps, syms, nve, div32, rows=B, lfinal=True):
    bits = torch.full((rows, codec.k_info), 7, dtype=torch.int32, device="cuda")
    lf = torch.full((rows, codec.k_info), np.nan, dtype=torch.float64, device="cuda")
    codec.demap_decode_device(syms[:rows], cons, bps, nve, bits, lfinal=lf if lfinal else None, div_f32=div32)
    torch.cuda.synchronize()
    return bits, lf


@pytest.mark.parametrize("cap", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fused_tiles_equal_two_launch_path(case, cap, prepared, monkeypatch):
    codec, cons, bps, syms, nve, div32, ref_bits, ref_lf = prepared(case, monkeypatch)
    _set_cap(monkeypatch, cap)
    bits, lf = _fused(codec, cons, bps, syms, nve, div32)
    if case.adv is None:
        assert torch.equal(bits, ref_bits)
        assert torch.equal(lf, ref_lf)   # (no NaN: torch.equal would refuse one)
        return
    # A NaN symbol poisons its own codeword only: every tile has rows the reference decodes to finite
    # values, they are finite here too, and the rest is equal with NaN == NaN
    clean = ~_poison(syms.cpu().numpy()).any(1)
    ref_fin = torch.isfinite(ref_lf).all(1).cpu().numpy()
    assert (ref_fin[clean]).all() and not ref_fin[~clean].all()
    tiles = np.arange(B) // 64
    assert all((clean & (tiles == t)).any() and (~clean & (tiles == t)).any() for t in range(10))
    assert torch.isfinite(lf[torch.from_numpy(clean).cuda()]).all()
    assert np.array_equal(bits.cpu().numpy(), ref_bits.cpu().numpy())
    np.testing.assert_array_equal(lf.cpu().numpy(), ref_lf.cpu().numpy())


@pytest.mark.parametrize("mod", list(KERNELS))
def test_three_tiles_on_one_wave(mod, prepared, monkeypatch):
    """B = 133 with one wave: static striding (3 < 4 x 1), the third tile in the first tile's buffer."""
    codec, cons, bps, syms, nve, div32, ref_bits, ref_lf = prepared(CASES[list(KERNELS).index(mod)], monkeypatch)
    _set_cap(monkeypatch, "1")
    bits, lf = _fused(codec, cons, bps, syms, nve, div32, rows=133)
    assert torch.equal(bits, ref_bits[:133])
    assert torch.equal(lf, ref_lf[:133])


@pytest.mark.parametrize("cap", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("mod", list(KERNELS))
def test_fused_tiles_without_lfinal(mod, cap, prepared, monkeypatch):
    codec, cons, bps, syms, nve, div32, ref_bits, _ = prepared(CASES[list(KERNELS).index(mod)], monkeypatch)
    _set_cap(monkeypatch, cap)
    bits, lf = _fused(codec, cons, bps, syms, nve, div32, lfinal=False)
    assert torch.equal(bits, ref_bits)
    assert torch.isnan(lf).all()   # the sentinel: nothing was written


def test_cap_leaves_unavailable_configurations_alone(monkeypatch):
    """With the cap set, a configuration without a fused kernel is still TDEC_EUNSUPPORTED at the
    C ABI and still falls back to the two launches in DevicePipeline."""
    monkeypatch.setenv(CAP, "2")
    codec = M.DVBRCS2_Turbo(212, "1/3")
    cons = D.constellation("64QAM")
    assert not codec.fused_available(cons, 6)
    _, syms, n0 = make_symbols(codec, 200, "64QAM", 3.0, 5, "cuda", want_info=False)
    _, div32, nve = D.demap_mode(np.complex64, cons.dtype, np.float64(n0))
    bits = torch.full((200, codec.k_info), 7, dtype=torch.int32, device="cuda")
    codec.reserve_fused(200)
    table = np.ascontiguousarray(cons.astype(np.complex64))
    rc = NT.lib().tdec_demap_decode_dev(codec.handle.h, 200, NT.ptr(syms), syms.shape[1], NT.ptr(table), 0, 64, 6,
                                        float(nve), int(div32), NT.ptr(bits), None,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == NT.TDEC_EUNSUPPORTED and (bits == 7).all()
    pipe = DevicePipeline(codec, "64QAM", 200, "cuda", fused=True)
    assert not pipe.fused
    out = pipe.run(syms, n0).clone()
    monkeypatch.delenv(CAP)
    ref = DevicePipeline(codec, "64QAM", 200, "cuda", fused=False).run(syms, n0)
    assert torch.equal(out, ref)
