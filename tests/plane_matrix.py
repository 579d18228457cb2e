"""Every (codec, modulation) of the tables for the kernels that write the decoder's
planes, and the planes they must write.

TEST INFRASTRUCTURE (a plain module like codec_matrix.py and harq_ref.py: numpy and the
C oracle only, no GPU, nothing imported from the kernels under test).  The plane
demappers' index arithmetic -- the chunk an item covers, the symbols that straddle a
chunk boundary, the LDS column of an LLR, the surplus bits of the last symbol, the zero
tail, k_demap_fix's dst table -- depends on (N, rate, bits per symbol), so
tests/test_gpu_plane_matrix.py runs every plane writer on all 28 x 6 = 168 combinations:

  CASES / CASE_IDS             (n, rate, modulation), codec_matrix.CODECS x MODS
  symbols(n, rate, mod)        complex64 [69, S], S = ceil(n_coded / bps): adversarial()'s
                               mixture, whose ties and non-finite symbols the split search
                               declines (so k_demap_fix runs on every split case); the last
                               symbol of every row finite and off-grid, a near-tie in every
                               fourth row of a split table (k_demap_fix then meets the
                               surplus bits too)
  maxlog_llr(syms, mod, nv, div_f32)
                               the host chain's LLRs in the decoder's sign, float64
                               [B, S * bps]: -oracle.demap on the symbols that are not NaN,
                               NaN for those that are
  reference_planes(llr64, n, punct, B)
                               the tile-layout float32 buffer those LLRs make, built on the
                               CPU from the restated de-puncture walk (harq_ref.walk), which
                               tests/test_plane_matrix_host.py pins to the oracle's own
                               de-puncture at every (N, rate)
  shape_facts(n, rate, mod)    what makes a case hard, from the walk and the codec's n_coded
"""
import functools

import numpy as np

import codec_matrix as CM
import harq_ref as H
from oracle import oracle as O
from modulations_amd import demap as D     # the label-ordered tables (python; no kernel)
from modulations_amd import tables as T

MODS = ("BPSK", "QPSK", "8PSK", "16QAM", "64QAM", "256QAM")
BPS = {mod: D.MODULATIONS[mod]["bps"] for mod in MODS}
SPLIT_MODS = ("16QAM", "64QAM", "256QAM")   # dm_split in tdec_demap_kernels.hip: square QAM, bps 4 / 6 / 8
ROWS = CM.ROWS                              # 69: one full 64-lane tile and a partial one of 5
CASES = [(n, rate, mod) for n, rate in CM.CODECS for mod in MODS]
CASE_IDS = [f"{CM.codec_id(n, rate)}-{mod}" for n, rate, mod in CASES]


def couples_per_item(bps):
    """dm_kc in tdec_demap_kernels.hip, restated: the couples one item of the plane
    demappers covers, 12 for QPSK and 16 for every other modulation."""
    return 12 if bps == 2 else 16


def n_symbols(n, rate, mod):
    """S = ceil(n_coded / bps) with the codec's advertised n_coded."""
    return -(-T.coded_size(n, T.PUNCTURE_PATTERNS[rate]) // BPS[mod])


def adversarial(cons, rng, shape):
    """Noisy points mixed with exact points, bisector ties, near-ties, far / tiny /
    huge values and NaN / inf, shuffled over the batch."""
    n = int(np.prod(shape))
    lv = np.unique(cons.real.astype(np.float64))
    mids = (lv[:-1] + lv[1:]) / 2
    k = n // 10
    parts = [cons[rng.integers(0, len(cons), n - 7 * k)] + 0.2 * (rng.standard_normal(n - 7 * k) +
                                                                 1j * rng.standard_normal(n - 7 * k)),
             cons[rng.integers(0, len(cons), k)],
             rng.choice(mids, k) + 1j * rng.choice(lv, k),
             rng.choice(mids, k) + 1j * rng.choice(mids, k),
             np.nextafter(rng.choice(mids, k), 9) + 1j * np.nextafter(rng.choice(mids, k), -9),
             10 * (rng.standard_normal(k) + 1j * rng.standard_normal(k)),
             1e-20 * (rng.standard_normal(k) + 1j * rng.standard_normal(k)),
             rng.choice(np.array([np.nan, np.inf, -np.inf + 1j, 1 + np.nan * 1j, 3e38 + 3e38j]), k)]
    s = np.concatenate(parts)
    rng.shuffle(s)
    return s.reshape(shape).astype(np.complex64)


def _seed(n, rate, mod, salt):
    num, den = (int(x) for x in rate.split("/"))
    return [salt, n, num, den, BPS[mod]]


@functools.lru_cache(maxsize=8)
def symbols(n, rate, mod):
    """complex64 [69, S] (read-only), seeded per case: adversarial()'s mixture, then the
    last symbol of every row replaced by a table point moved off the grid by a quarter
    of the smallest level spacing in both axes (finite, no tie, every LLR non-zero), so
    that surplus bits of the last symbol that were not cut would show; in every fourth row
    of a split table by a near-tie with the same properties."""
    cons = D.constellation(mod)
    rng = np.random.default_rng(_seed(n, rate, mod, 168))
    s = adversarial(cons, rng, (ROWS, n_symbols(n, rate, mod)))
    lv = np.unique(np.concatenate([cons.real, cons.imag]).astype(np.float32).astype(np.float64))
    q = np.diff(lv).min() / 4
    s[:, -1] = (cons[rng.integers(0, len(cons), ROWS)] + q * (1 + 1j)).astype(np.complex64)
    if mod in SPLIT_MODS:
        # every fourth row ends on a near-tie instead: four float32 steps beside the outermost
        # bisector, a quarter spacing off a level in the other axis.  Finite, off-grid and no
        # LLR zero as well, but the split search declines it, so k_demap_fix meets the last
        # symbol and its surplus bits
        near = np.float32((lv[-2] + lv[-1]) / 2)
        for _ in range(4):
            near = np.nextafter(near, np.float32(9))
        s[3::4, -1] = near + 1j * (rng.choice(lv, len(s[3::4])) + q).astype(np.float32)
    s.setflags(write=False)
    return s


def tie_count(syms, mod):
    """Finite symbols whose two nearest table points are exactly equally far in float64."""
    cons = D.constellation(mod).astype(np.complex128)
    z = syms.reshape(-1).astype(np.complex128)
    z = z[np.isfinite(z.real) & np.isfinite(z.imag)]
    d = np.sort((z.real[:, None] - cons.real[None, :]) ** 2 + (z.imag[:, None] - cons.imag[None, :]) ** 2, axis=1)
    return int((d[:, 0] == d[:, 1]).sum())


def maxlog_llr(syms, mod, nv, div_f32):
    """float64 [B, S * bps], decoder sign: the host chain (oracle.demap, negated) on the
    symbols that are not NaN, NaN for the LLRs of those that are."""
    cons, bps = D.constellation(mod), BPS[mod]
    flat = syms.reshape(-1)
    llr = np.full(flat.size * bps, np.nan, np.float64)
    fin = ~np.isnan(flat)
    llr.reshape(-1, bps)[fin] = (-O.demap(flat[fin], cons, bps, nv, div_f32=div_f32)).reshape(-1, bps)
    return llr.reshape(syms.shape[0], -1)


def reference_planes(llr64, n, punct, B):
    """The float32 tile-layout buffer (harq_ref.to_tiles; ceil(B / 64) tiles) the rows
    llr64 [B, any length] de-puncture into: the LLRs rounded to float32, copied through
    the restated walk (a plain indexed copy: -0.0 and NaN survive), 0.0 for what the
    pattern does not send, for LLR indices >= min(row length, walk), and for the idle
    lanes of the last tile."""
    llr64 = np.asarray(llr64)
    assert llr64.ndim == 2 and llr64.shape[0] == B
    src, length = H.walk(n, punct)
    n_avail = min(llr64.shape[1], length)
    with np.errstate(invalid="ignore", over="ignore"):
        l32 = llr64[:, :n_avail].astype(np.float32)
    planes6 = np.zeros((B, n, 6), np.float32)
    for comp in range(6):
        k = np.nonzero((src[comp] >= 0) & (src[comp] < n_avail))[0]
        planes6[:, k, comp] = l32[:, src[comp][k]]
    return H.to_tiles(planes6, fill=0.0)


def shape_facts(n, rate, mod):
    """What the case exercises, from the walk and the codec's real n_coded:
      straddled  chunk boundaries (multiples of couples_per_item below N) whose first LLR
                 is not a symbol's first bit and lies inside the symbols sent: that
                 symbol is demapped by two items
      surplus    S * bps - walk where positive: bits of the last symbol to drop
      padding    walk - n_coded where positive (rate 2/3 with 3 not dividing N)
      zero_tail  walk - S * bps where positive: LLRs of the walk no symbol provides
      ragged     N is no multiple of couples_per_item: the last chunk is short."""
    punct = T.PUNCTURE_PATTERNS[rate]
    bps = BPS[mod]
    src, length = H.walk(n, punct)
    n_coded = T.coded_size(n, punct)
    S = -(-n_coded // bps)
    kc = couples_per_item(bps)
    off = src[0]                                   # the LLR index of A of couple k: where couple k starts
    cuts = off[np.arange(kc, n, kc)]
    return {"straddled": int(((cuts % bps != 0) & (cuts < min(S * bps, length))).sum()),
            "surplus": max(0, S * bps - length), "padding": max(0, length - n_coded),
            "zero_tail": max(0, length - S * bps), "ragged": n % kc != 0}
