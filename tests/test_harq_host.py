"""Hybrid ARQ, host side: the redundancy versions, the restated
soft combining (harq_ref.py) against the C oracle, and the C ABI's bookkeeping.  No GPU."""
import os
import re

import numpy as np
import pytest

import harq_ref as H
from oracle import oracle as O
from modulations_amd import _native
from modulations_amd import tables as T
from modulations_amd.dvb_rcs2_turbo import DVBRCS2_Turbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = ("1/2", "2/3", "3/4")
VERSIONS = [(rate, rv) for rate in RATES for rv in range(T.PUNCTURE_PATTERNS[rate]["period"])]
TAB, G = O.trellis()

# what all versions of a rate send between them, (row, phase): rate 1/2 all four parity rows
# at both phases; rates 2/3 and 3/4 never send Y2, and every other row at every phase
UNION = {
    "1/2": {(r, p) for r in ("W1", "Y1", "W2", "Y2") for p in range(2)},
    "2/3": {(r, p) for r in ("W1", "Y1", "W2") for p in range(3)},
    "3/4": {(r, p) for r in ("W1", "Y1", "W2") for p in range(4)},
}
# LLRs the walk of EVERY version reads: rate 1/2 sends two parities at each phase (4 per
# couple); rate 2/3 one at each of its three phases (3 per couple, so 3 N also where 3 does
# not divide N: the versions' walks are as long as each other); rate 3/4 three per four couples
CONSUMED = {("1/2", 48): 192, ("1/2", 212): 848, ("1/2", 752): 3008,
            ("2/3", 48): 144, ("2/3", 212): 636, ("2/3", 752): 2256,
            ("3/4", 48): 132, ("3/4", 212): 583, ("3/4", 752): 2068}


def test_rv0_is_the_tables_pattern():
    for rate, p in T.PUNCTURE_PATTERNS.items():
        assert T.redundancy_version(p, 0) == p
        assert H.redundancy_version(p, 0) == p
        c = DVBRCS2_Turbo(48, rate)
        assert c.rv == 0 and c.punct == p and c.n_coded == T.coded_size(48, p)


@pytest.mark.parametrize("rate,rv", VERSIONS)
def test_versions_match_the_restatement(rate, rv):
    p = T.PUNCTURE_PATTERNS[rate]
    got = T.redundancy_version(p, rv)
    assert got == H.redundancy_version(p, rv)
    for key in H.ROWS:
        assert got[key] == [p[key][(ph + rv) % p["period"]] for ph in range(p["period"])]
    c = DVBRCS2_Turbo(212, rate, rv=rv)
    assert c.rv == rv and c.punct == got
    assert c.n_coded == T.coded_size(212, got) and c._enc_len() == H.walk(212, got)[1]


@pytest.mark.parametrize("rate", RATES)
def test_union_of_the_versions(rate):
    p = T.PUNCTURE_PATTERNS[rate]
    sent = [H.transmitted(T.redundancy_version(p, rv)) for rv in range(p["period"])]
    assert set().union(*sent) == UNION[rate]
    # each (row, phase) of the union is sent by exactly as many versions as the row has ones
    for row, ph in UNION[rate]:
        assert sum((row, ph) in s for s in sent) == sum(p[row])


@pytest.mark.parametrize("rate,rv", VERSIONS)
@pytest.mark.parametrize("n", [48, 212, 752])
def test_consumed_size_of_every_version(rate, rv, n):
    p = T.redundancy_version(T.PUNCTURE_PATTERNS[rate], rv)
    assert T.consumed_size(n, p) == CONSUMED[rate, n] == H.walk(n, p)[1]


def test_out_of_range_versions_are_refused():
    for rate, p in T.PUNCTURE_PATTERNS.items():
        for rv in (-1, p["period"]):
            with pytest.raises(ValueError):
                T.redundancy_version(p, rv)
            with pytest.raises(ValueError):
                DVBRCS2_Turbo(48, rate, rv=rv)


def test_tile_layout_round_trip():
    rng = np.random.default_rng(5)
    p6 = rng.standard_normal((70, 12, 6)).astype(np.float32)
    flat = H.to_tiles(p6, fill=7.0)
    assert flat.shape == (2 * H.tile_floats(12),)
    assert np.array_equal(H.from_tiles(flat, 70, 12), p6)
    # slot 65 (tile 1, lane 1), step 3: float4 at [k][lane], float2 behind the tile's float4s
    t1 = flat[H.tile_floats(12):]
    assert np.array_equal(t1[(3 * 64 + 1) * 4:(3 * 64 + 1) * 4 + 4], p6[65, 3, :4])
    assert np.array_equal(t1[12 * 64 * 4 + (3 * 64 + 1) * 2:12 * 64 * 4 + (3 * 64 + 1) * 2 + 2], p6[65, 3, 4:])
    assert np.all(t1.reshape(-1)[(0 * 64 + 6) * 4:(0 * 64 + 6) * 4 + 4] == 7.0)   # an idle lane


@pytest.mark.parametrize("rate,rv", VERSIONS + [("1/3", 0)])
@pytest.mark.parametrize("n", [48, 212])
def test_one_transmission_onto_zero_planes_is_the_oracles_depuncture(rate, rv, n):
    p = T.redundancy_version(T.PUNCTURE_PATTERNS[rate], rv)
    rng = np.random.default_rng([n, rv, RATES.index(rate) if rate in RATES else 9])
    llr = rng.standard_normal((3, H.walk(n, p)[1] + 5)).astype(np.float32)
    got = H.accumulate(np.zeros((3, n, 6), np.float32), llr, n, p)
    for r in range(3):
        want = O.depuncture(llr[r], n, p["period"], T.puncture_matrix(p))      # [6][n]
        assert np.array_equal(got[r], want.T)


def test_accumulate_rules():
    """Add order, float64 rows rounded first, untransmitted components and unselected slots
    untouched bit for bit, inf + -inf = NaN."""
    n, p = 48, T.redundancy_version(T.PUNCTURE_PATTERNS["3/4"], 1)
    src, length = H.walk(n, p)
    rng = np.random.default_rng(11)
    start = rng.standard_normal((5, n, 6)).astype(np.float32)
    start[0, 0, :] = [-0.0, np.inf, -0.0, -0.0, -0.0, -0.0]
    llr = rng.standard_normal((3, length)) * 1e3
    llr[2, src[1, 0]] = -np.inf
    row_of = np.array([2, -1, 0, 3, 1])
    got = H.accumulate(start.copy(), llr, n, p, row_of)
    assert H.same_bits(got[[1, 3]], start[[1, 3]])                          # -1 and an entry >= rows
    assert np.isnan(got[0, 0, 1])
    off = src < 0                                                           # [6][n] not transmitted
    assert off[5].all() and off[2:].sum() == 3 * n + n // 4                 # Y2 never, W1 / Y1 / W2 at one phase in four
    for c in (0, 2, 4):
        assert H.same_bits(got[c].T[off], start[c].T[off])
    want = start[2, 7, 0] + np.float32(llr[0, src[0, 7]])
    assert got[2, 7, 0] == want and got.dtype == np.float32
    # the order of the calls is the order of the sums
    a = H.accumulate(H.accumulate(start.copy(), llr, n, p, row_of), 1e-4 * llr, n, p, row_of)
    b = H.accumulate(H.accumulate(start.copy(), 1e-4 * llr, n, p, row_of), llr, n, p, row_of)
    assert not H.same_bits(a, b)


def _codec_args(n, punct):
    perm = T.interleaver(n)
    return punct["period"], T.puncture_matrix(punct), 8, perm, T.inverse_interleaver(perm, "stable"), TAB


def test_chase_planes_are_a_rate_third_vector():
    """T summed transmissions of a rate-1/2 codec, read back from the restated planes, decoded
    by the rate-1/3 oracle = the rate-1/2 oracle on the sums (punctured positions are zero LLRs
    to both)."""
    n, p, third = 48, T.PUNCTURE_PATTERNS["1/2"], T.PUNCTURE_PATTERNS["1/3"]
    rng = np.random.default_rng(3)
    tx = [rng.standard_normal((9, H.walk(n, p)[1])).astype(np.float32) * 2 for _ in range(3)]
    p6 = np.zeros((9, n, 6), np.float32)
    for llr in tx:
        H.accumulate(p6, llr, n, p)
    summed = (tx[0] + tx[1]) + tx[2]
    a = O.decode_batch(H.llr6(p6), n, *_codec_args(n, third), want_lfinal=True)
    b = O.decode_batch(summed, n, *_codec_args(n, p), want_lfinal=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_all_versions_fill_every_parity_the_rate_sends():
    n, rate = 48, "3/4"
    p6 = np.zeros((2, n, 6), np.float32)
    for rv in range(4):
        p = T.redundancy_version(T.PUNCTURE_PATTERNS[rate], rv)
        H.accumulate(p6, np.ones((2, H.walk(n, p)[1]), np.float32), n, p)
    assert np.array_equal(p6[0], np.tile(np.float32([4, 4, 1, 1, 1, 0]), (n, 1)))


# ---- the C ABI's bookkeeping ---------------------------------------------------------------

def _harq_header_symbols():
    src = open(os.path.join(ROOT, "include", "harq.h")).read()
    return sorted(set(re.findall(r"^\s*(?:[\w\s\*]+?)\b(harq_\w+)\s*\(", src, re.M)))


def test_harq_header_matches_binding_list():
    assert _harq_header_symbols() == sorted(_native.HARQ_EXPORTS)
    assert not any(name.startswith("tdec_") for name in _native.HARQ_EXPORTS)
    assert not set(_native.HARQ_EXPORTS) & set(_native.EXPORTS)
    assert len(_native.EXPORTS) == 67                                              # as before hybrid ARQ
    src = open(os.path.join(ROOT, "include", "harq.h")).read()
    assert not re.findall(r"^\s*(?:[\w\s\*]+?)\b(tdec_\w+)\s*\(", src, re.M)    # harq.h declares no tdec_ call


def test_library_exports_the_harq_symbols():
    import ctypes as C
    import subprocess
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in _native.HARQ_EXPORTS:
        assert re.search(rf"\bT {name}$", out, re.M), name
        f = getattr(lib, name)
        assert f.restype is C.c_int and f.argtypes[0] is C.c_void_p
    assert [a.__name__ for a in lib.harq_depuncture_acc_dev.argtypes] == \
        ["c_void_p", "c_int", "c_void_p", "c_int", "c_long", "c_int", "c_void_p", "c_void_p", "c_void_p"]
    assert [a.__name__ for a in lib.harq_workload_tx_dev.argtypes] == \
        ["c_void_p", "c_int", "c_int", "c_long", "c_ulong", "c_void_p", "c_int", "c_int", "c_double", "c_int",
         "c_double", "c_int", "c_void_p", "c_void_p", "c_void_p", "c_void_p"]


def test_pipeline_refuses_codecs_of_another_code():
    from modulations_amd.workload import HarqPipeline
    mother = DVBRCS2_Turbo(48, "1/3", inv_perm="stable")
    other_n = DVBRCS2_Turbo(64, "1/2", inv_perm="stable")
    other_perm = DVBRCS2_Turbo(48, "1/2", interleaver="valid-perm")
    other_inv = DVBRCS2_Turbo(48, "1/2", inv_perm=np.roll(mother.inv_perm, 1))
    for bad in (other_n, other_perm, other_inv):
        with pytest.raises(ValueError):
            HarqPipeline([bad], mother, "QPSK", 4, "cpu")
    with pytest.raises(ValueError):
        HarqPipeline([], mother, "QPSK", 4, "cpu")
