"""The inputs of tests/test_gpu_codec_matrix.py, checked on the CPU: the codec
list is the tables' own, the fixed batch's rows are as long as the de-puncture
walk, and the early-stop batch makes lanes of one wave end on different trips for
every (codec, algorithm) pair (codec_matrix.es_condition) -- a condition on the
inputs by the restated rule (early_stop_ref.py), never by a GPU result."""
import numpy as np
import pytest

import codec_matrix as CM
from modulations_amd import tables as T

IDS = [CM.codec_id(*c) for c in CM.CODECS]


def test_codecs_are_the_tables():
    assert len(CM.CODECS) == 28 == len(set(CM.CODECS))
    assert {n for n, _ in CM.CODECS} == set(T.INTERLEAVER_PARAMS)
    assert {r for _, r in CM.CODECS} == set(T.PUNCTURE_PATTERNS)


@pytest.mark.parametrize("n,rate", CM.CODECS, ids=IDS)
def test_fixed_batch_shape(n, rate):
    punct = T.PUNCTURE_PATTERNS[rate]
    info, llr = CM.fixed_batch(n, rate)
    assert info.shape == (CM.ROWS, 2 * n) and CM.ROWS == 64 + 5
    assert llr.dtype == np.float32 and llr.shape == (CM.ROWS, T.consumed_size(n, punct))
    assert np.isfinite(llr).all()
    # rows are longer than n_coded exactly where the period does not divide N (the rate-2/3 quirk)
    assert (llr.shape[1] > T.coded_size(n, punct)) == (n % punct["period"] != 0)
    assert llr.shape[1] >= T.coded_size(n, punct)
    assert not llr[CM.ZERO_ROW].any()
    clean = llr[CM.CLEAN_ROW]
    assert set(np.abs(clean).tolist()) <= {0.0, 20.0} and (np.abs(clean) == 20.0).sum() >= T.coded_size(n, punct)
    # a noise scale of its own per row: the rows' spreads differ
    other = np.delete(np.arange(CM.ROWS), [CM.ZERO_ROW, CM.CLEAN_ROW])
    spread = llr[other].std(axis=1)
    assert spread.max() > 1.3 * spread.min()
    # seeded: a second build gives the same rows, and the arrays handed out are read-only
    CM.fixed_batch.cache_clear()
    again = CM.fixed_batch(n, rate)
    assert np.array_equal(again[0], info) and np.array_equal(again[1], llr)
    assert not again[1].flags.writeable
    w = CM.wide(llr)
    assert w.shape == (CM.ROWS, llr.shape[1] + 7) and np.array_equal(w[:, :llr.shape[1]], llr)
    assert np.isnan(w[:, llr.shape[1]:]).all()


@pytest.mark.parametrize("n,rate", CM.CODECS, ids=IDS)
def test_early_stop_batch_shape(n, rate):
    punct = T.PUNCTURE_PATTERNS[rate]
    info, llr = CM.early_stop_batch(n, rate)
    assert info.shape == (CM.ROWS, 2 * n)
    assert llr.dtype == np.float32 and llr.shape == (CM.ROWS, T.consumed_size(n, punct))
    perm, inv = CM.interleaver(n, "valid-perm")
    assert np.array_equal(np.sort(perm), np.arange(n)) and np.array_equal(perm[inv], np.arange(n))


@pytest.mark.parametrize("algo", CM.ALGOS)
@pytest.mark.parametrize("n,rate", CM.CODECS, ids=IDS)
def test_early_stop_rows_end_on_different_iterations(n, rate, algo):
    """At least three distinct iteration counts over the 69 rows, the cap (8) and
    one of 3 or fewer among them."""
    bits, lf, n_iter = CM.early_stop_ref(n, rate, algo)
    assert n_iter.shape == (CM.ROWS,) and n_iter.min() >= 2 and n_iter.max() <= CM.ITERATIONS
    hist = np.bincount(n_iter, minlength=CM.ITERATIONS + 1).tolist()
    assert CM.es_condition(n_iter), hist
    assert CM.early_stop_ref(n, rate, algo)[2] is n_iter   # computed once per key
