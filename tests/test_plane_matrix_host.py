"""tests/plane_matrix.py checked on the CPU: the restated de-puncture walk against the
oracle's own at every (N, rate), and the conditions that keep a case of
tests/test_gpu_plane_matrix.py from passing trivially.

Measured over the 168 (codec, modulation) cases, with the codecs' real n_coded
(shape_facts; asserted in test_matrix_totals):

  42  have at least one chunk boundary inside a symbol (610 such boundaries in all):
      QPSK 7 (rate 3/4), 8PSK 14 and 64QAM 14 (rates 1/2 and 3/4), 256QAM 7 (rate 3/4).
      BPSK has none, and neither has 16QAM: 16 couples carry 96, 64, 48 or 44 LLRs at
      rates 1/3, 1/2, 2/3 and 3/4 (the last two send the same number in every 16
      couples although their periods are 3 and 4), all multiples of 4, so no boundary
      of a 16QAM item can fall inside a symbol at any codec of the tables
  36  have surplus bits in the last symbol
  36  are padded (rate 2/3 with 3 not dividing N: 6 codecs x 6 modulations); in 25 of
      them the symbols end before the walk does and the tail must be zero
  21  (N, modulation) pairs, 84 cases, have a ragged last chunk (N = 212, 220, 424 for
      every modulation but QPSK; 64, 212, 220, 424, 752, 848 for QPSK, whose items are
      12 couples)
"""
import numpy as np
import pytest

import codec_matrix as CM
import harq_ref as H
import plane_matrix as PM
from oracle import oracle as O
from modulations_amd import demap as D
from modulations_amd import tables as T

CODEC_IDS = [CM.codec_id(*c) for c in CM.CODECS]


@pytest.mark.parametrize("n,rate", CM.CODECS, ids=CODEC_IDS)
def test_walk_restatement_equals_the_oracles_depuncture(n, rate):
    """Three random rows: decoding the punctured rows equals decoding, as the rate-1/3
    mother code, the 6N LLRs read back from reference_planes -- bits and L_final, IEEE
    ==.  The GPU comparisons are then against planes independent of k_depuncture."""
    punct = T.PUNCTURE_PATTERNS[rate]
    third = T.PUNCTURE_PATTERNS["1/3"]
    rng = np.random.default_rng([28, n, CM.CODECS.index((n, rate))])
    w = CM.walk(n, rate)
    llr = (2.5 * rng.standard_normal((3, w))).astype(np.float32)
    perm, inv = CM.interleaver(n, "reference")
    want = O.decode_batch(llr, n, punct["period"], T.puncture_matrix(punct), 2, perm, inv, CM.TAB, want_lfinal=True)
    tiles = PM.reference_planes(llr.astype(np.float64), n, punct, 3)
    assert tiles.shape == (H.tile_floats(n),) and tiles.dtype == np.float32
    planes6 = H.from_tiles(tiles, 3, n)
    assert np.count_nonzero(planes6) == 3 * w                      # every LLR of the walk landed once
    assert not H.from_tiles(tiles, 64, n)[3:].any()                # idle lanes are zero
    got = O.decode_batch(H.llr6(planes6), n, 1, T.puncture_matrix(third), 2, perm, inv, CM.TAB, want_lfinal=True)
    assert np.array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert np.abs(want[1]).max() > 0


def test_reference_planes_cuts_and_keeps_what_it_should():
    n, punct = 48, T.PUNCTURE_PATTERNS["1/2"]
    src, w = H.walk(n, punct)
    llr = np.arange(1, w + 4, dtype=np.float64)[None, :].repeat(2, axis=0)   # 3 surplus columns
    llr[0, 5] = -0.0
    llr[1, 7] = np.nan
    p = H.from_tiles(PM.reference_planes(llr, n, punct, 2), 2, n)
    for comp in range(6):
        sent = src[comp] >= 0
        assert np.array_equal(p[0, sent, comp], llr[0, src[comp][sent]].astype(np.float32))
        assert not p[:, ~sent, comp].any()
    assert np.signbit(p[0][(src == 5).T]).all() and np.isnan(p[1][(src == 7).T]).all()
    short = H.from_tiles(PM.reference_planes(llr[:, :w - 10], n, punct, 2), 2, n)
    assert not short[0][(src >= w - 10).T].any()                   # LLR indices the rows do not reach: 0.0
    assert np.array_equal(short[0][(src < w - 10).T], p[0][(src < w - 10).T])


def test_matrix_totals():
    """The conditions the matrix must contain, and the totals of the module docstring."""
    assert len(PM.CASES) == 168 and len(set(PM.CASE_IDS)) == 168
    facts = {c: PM.shape_facts(*c) for c in PM.CASES}
    straddled = {mod: sum(1 for c, f in facts.items() if c[2] == mod and f["straddled"]) for mod in PM.MODS}
    assert straddled == {"BPSK": 0, "QPSK": 7, "8PSK": 14, "16QAM": 0, "64QAM": 14, "256QAM": 7}, straddled
    # every modulation that can straddle does (16QAM cannot: the module docstring)
    assert all(straddled[mod] >= 1 for mod in PM.MODS if mod not in ("BPSK", "16QAM"))
    for rate, per16 in (("1/3", 96), ("1/2", 64), ("2/3", 48), ("3/4", 44)):
        for n in T.INTERLEAVER_PARAMS:
            off = H.walk(n, T.PUNCTURE_PATTERNS[rate])[0][0]
            assert np.all(off[np.arange(16, n, 16)] == per16 * np.arange(1, (n - 1) // 16 + 1)) and per16 % 4 == 0
    assert sum(f["straddled"] for f in facts.values()) == 610
    surplus = sum(1 for f in facts.values() if f["surplus"])
    assert surplus == 36 and surplus >= 30
    padded = [c for c, f in facts.items() if f["padding"]]
    assert len(padded) == 36 and {c[1] for c in padded} == {"2/3"} and all(c[0] % 3 for c in padded)
    assert sum(1 for f in facts.values() if f["zero_tail"]) == 25
    ragged = {(c[0], c[2]) for c, f in facts.items() if f["ragged"]}
    assert len(ragged) == 21 and sum(1 for f in facts.values() if f["ragged"]) == 84
    for mod in PM.SPLIT_MODS:
        assert any(m == mod for _, m in ragged)
    # a surplus bit is never counted where the symbols do not even reach the walk
    assert not any(f["surplus"] and f["zero_tail"] for f in facts.values())


def test_chunk_sizes_restate_dm_kc():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "modulations_amd", "csrc", "tdec_demap_kernels.hip")) as f:
        text = f.read()
    assert re.search(r"constexpr int DM_KC = 16;", text)
    assert re.search(r"constexpr int dm_kc\(int bps\) \{ return bps == 2 \? 12 : DM_KC; \}", text)
    assert [PM.couples_per_item(b) for b in (1, 2, 3, 4, 6, 8)] == [16, 12, 16, 16, 16, 16]


@pytest.mark.parametrize("n,rate,mod", PM.CASES, ids=PM.CASE_IDS)
def test_symbols_contain_what_the_split_search_declines(n, rate, mod):
    s = PM.symbols(n, rate, mod)
    assert s.dtype == np.complex64 and s.shape == (PM.ROWS, PM.n_symbols(n, rate, mod)) and not s.flags.writeable
    assert PM.tie_count(s, mod) > 0
    assert np.isnan(s).any() and (np.isinf(s.real) | np.isinf(s.imag)).any()
    last = s[:, -1]
    assert np.isfinite(last.real).all() and np.isfinite(last.imag).all()
    assert PM.tie_count(last, mod) == 0
    # off-grid: every LLR of the last symbol is non-zero
    assert np.all(PM.maxlog_llr(last[:, None], mod, 0.04, False) != 0)
    if mod in PM.SPLIT_MODS:   # every fourth row ends a few float32 steps beside a bisector: declined, yet finite
        lv = np.unique(D.constellation(mod).real.astype(np.float64))
        gap = last[3::4].real.astype(np.float64) - (lv[-2] + lv[-1]) / 2
        assert len(gap) >= 16 and np.all((gap > 0) & (gap < 1e-6))
    assert s is PM.symbols(n, rate, mod)
