"""One small batch per codec of the tables, and its references, shared by every
route's test.

TEST INFRASTRUCTURE (a plain module, like merge_fixtures.py and rx_patterns.py:
numpy and the C oracle only, no GPU).  The codec table has 7 block sizes and 4
puncturing rates; the de-puncture walk, perm's image, the used-position list, the
checkpoint raggedness (N % 8 = 4 at 212 and 220) and the LDS plans all depend on
(N, rate), so tests/test_gpu_codec_matrix.py runs every decoder on every one of the
28 codecs, in both algorithms, on the batches built here:

  fixed_batch(n, rate)        69 rows (a full 64-lane tile plus 5) for the fixed
                              8-iteration decode, reference interleaver,
                              inv_perm="stable";
  wide(llr)                   the same rows in a wider buffer whose surplus columns
                              are NaN (decode() stops reading at the end of the walk);
  early_stop_batch(n, rate)   69 rows for the early-stop decoders, valid-perm,
                              Eb/N0 ramped over the rows so that lanes of one wave
                              end on different iterations.

The references -- oracle.decode_batch and the restated early-stop rule
(early_stop_ref.py) -- are computed once per (n, rate, algo) and cached; every array
handed out is read-only.  log-MAP references depend on whether the oracle's
primitives are pinned to a device's tables (conftest.trans_tables), so that state is
part of their cache key.
"""
import functools

import numpy as np

import early_stop_ref as R
from oracle import oracle as O
from modulations_amd import tables as T

CODECS = [(n, rate) for n in T.INTERLEAVER_PARAMS for rate in T.PUNCTURE_PATTERNS]
ALGOS = ("max-log", "log-map")
ROWS = 69            # one full tile of 64 lanes and a partial one of 5
ZERO_ROW = 5         # all zeros: ties everywhere
CLEAN_ROW = 6        # noise-free +-20
ITERATIONS = 8
ES_MIN_DISTINCT = 3  # the condition on early_stop_batch (es_condition)

# Eb/N0 (dB) of the first and last row of early_stop_batch: 0 to 6 dB.  The two short
# blocks decode (or give up) too quickly there for log-MAP to reach the cap, so
# their ramp starts at -3 dB.
ES_RAMP_DB = {n: (0.0, 6.0) if n >= 212 else (-3.0, 6.0) for n in T.INTERLEAVER_PARAMS}
# Seeds of early_stop_batch (0 where none is listed), found on the CPU by running the
# restated rule on build_early_stop_batch(n, rate, seed, ramp) for seed = 0, 1, ...:
# the first seed whose iteration counts meet es_condition in both algorithms with two
# rows at the cap and two at 3 or fewer (one of each at (48, 3/4), (64, 2/3) and
# (64, 3/4), where no seed below 48 gave two).
# tests/test_codec_matrix_host.py asserts the condition for all 56 (codec, algorithm) pairs.
ES_SEEDS = {(48, "1/3"): 24, (48, "1/2"): 32, (48, "2/3"): 14, (64, "1/2"): 3, (64, "2/3"): 1, (64, "3/4"): 5,
            (212, "1/3"): 1, (212, "2/3"): 1, (220, "2/3"): 6, (220, "3/4"): 2, (424, "2/3"): 1, (752, "3/4"): 2}

TAB, G = O.trellis()


def codec_id(n, rate):
    return f"{n}-{rate.replace('/', '_')}"


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _seed(n, rate, salt):
    num, den = (int(x) for x in rate.split("/"))
    return [salt, n, num, den]


def walk(n, rate):
    """LLRs per codeword that decode()'s de-puncture loop reads."""
    return T.consumed_size(n, T.PUNCTURE_PATTERNS[rate])


def interleaver(n, kind):
    """(perm, inv_perm) as DVBRCS2_Turbo builds them for interleaver=kind
    ("reference" with inv_perm="stable", or "valid-perm")."""
    if kind == "reference":
        perm = T.interleaver(n)
        return perm, T.inverse_interleaver(perm, "stable")
    perm = T.valid_interleaver(n)
    return perm, np.argsort(perm).astype(np.int32)


def oracle_encode(info, n, rate, perm):
    """encode() of every row (the oracle's, pinned to the reference's by
    tests/test_oracle_golden.py): int32 [B, encode()'s own length]."""
    punct = T.PUNCTURE_PATTERNS[rate]
    pm = T.puncture_matrix(punct)
    return np.stack([O.encode(b, n, punct["period"], pm, perm, TAB, G) for b in info])


def _pad_to_walk(llr, n, rate):
    w = walk(n, rate)
    return np.pad(llr, ((0, 0), (0, w - llr.shape[1]))) if llr.shape[1] < w else llr


@functools.lru_cache(maxsize=None)
def fixed_batch(n, rate):
    """(info int32 [69, 2N], llr float32 [69, walk]): noisy encoded LLRs, amplitude 2
    with a noise scale of its own per row (0.5 to 3), zero-padded to the walk where
    encode() is shorter (rate 2/3 where 3 does not divide N); row ZERO_ROW all
    zeros, row CLEAN_ROW noise-free +-20.  Seeded per codec."""
    rng = np.random.default_rng(_seed(n, rate, 69))
    perm, _ = interleaver(n, "reference")
    info = rng.integers(0, 2, (ROWS, 2 * n)).astype(np.int32)
    x = 1.0 - 2.0 * oracle_encode(info, n, rate, perm)
    sigma = rng.uniform(0.5, 3.0, (ROWS, 1))
    llr = (2.0 * x + sigma * rng.standard_normal(x.shape)).astype(np.float32)
    llr[ZERO_ROW] = 0.0
    llr[CLEAN_ROW] = (20.0 * x[CLEAN_ROW]).astype(np.float32)
    return _ro(info, np.ascontiguousarray(_pad_to_walk(llr, n, rate)))


def wide(llr, surplus=7):
    """The rows of llr at the start of a [B, walk + surplus] buffer whose other
    columns are NaN: rows a caller hands over with a stride longer than the walk."""
    out = np.full((llr.shape[0], llr.shape[1] + surplus), np.nan, np.float32)
    out[:, :llr.shape[1]] = llr
    return out


def build_early_stop_batch(n, rate, seed, ramp_db):
    """early_stop_batch for one seed and one (first, last) Eb/N0 in dB."""
    rng = np.random.default_rng(_seed(n, rate, seed))
    perm, _ = interleaver(n, "valid-perm")
    info = rng.integers(0, 2, (ROWS, 2 * n)).astype(np.int32)
    coded = oracle_encode(info, n, rate, perm)
    llr = R.bpsk_channel(coded, 2 * n, rng, np.linspace(*ramp_db, ROWS))
    return info, np.ascontiguousarray(_pad_to_walk(llr, n, rate))


@functools.lru_cache(maxsize=None)
def early_stop_batch(n, rate):
    """(info [69, 2N], llr float32 [69, walk]) for interleaver="valid-perm": BPSK
    LLRs (early_stop_ref.bpsk_channel) with Eb/N0 ramped linearly over the rows
    between ES_RAMP_DB[n], zero-padded to the walk.  Seeded per codec (ES_SEEDS)."""
    return _ro(*build_early_stop_batch(n, rate, ES_SEEDS.get((n, rate), 0), ES_RAMP_DB[n]))


def _algo(algo):
    return ALGOS.index(algo) if isinstance(algo, str) else int(algo)


def _prims(algo):
    """The part of a reference's cache key that says which log-MAP primitives the
    oracle had (max-log has none)."""
    return bool(_algo(algo)) and O.trans_pinned()


@functools.lru_cache(maxsize=None)
def _fixed_ref(n, rate, algo, prims):
    punct = T.PUNCTURE_PATTERNS[rate]
    perm, inv = interleaver(n, "reference")
    return _ro(*O.decode_batch(fixed_batch(n, rate)[1], n, punct["period"], T.puncture_matrix(punct), ITERATIONS,
                               perm, inv, TAB, algo=algo, want_lfinal=True))


def fixed_ref(n, rate, algo):
    """(bits int32 [69, 2N], L_final f64 [69, 2N]) of fixed_batch by the oracle."""
    return _fixed_ref(n, rate, _algo(algo), _prims(algo))


@functools.lru_cache(maxsize=None)
def _early_stop_ref(n, rate, algo, prims):
    perm, inv = interleaver(n, "valid-perm")
    return _ro(*R.decode_early_stop_batch(early_stop_batch(n, rate)[1], n, T.PUNCTURE_PATTERNS[rate], ITERATIONS,
                                          perm, inv, TAB, algo))


def early_stop_ref(n, rate, algo):
    """(bits, L_final, n_iter int32 [69]) of early_stop_batch by the restated rule."""
    return _early_stop_ref(n, rate, _algo(algo), _prims(algo))


def es_condition(n_iter):
    """The condition that keeps an early-stop case from passing trivially: the
    rows' iteration counts take at least ES_MIN_DISTINCT distinct values, the cap
    among them and one of 3 or fewer (lanes of one wave end on different trips,
    some early, some never)."""
    v = set(np.asarray(n_iter).tolist())
    return len(v) >= ES_MIN_DISTINCT and ITERATIONS in v and min(v) <= 3
