"""The early-stop rule on the CPU (tests/early_stop_ref.py): the numpy
restatement is pinned to the oracle's fixed-iteration decode, runs to the cap where
the decisions never settle, stops at mixed counts at low SNR, and the Python
keyword refuses cleanly where the frame decoder is not available."""
import numpy as np
import pytest

import early_stop_ref as R
from oracle import oracle as O
from modulations_amd import dvb_rcs2_turbo as M
from modulations_amd import tables as T

TAB, _ = O.trellis()
I = 8


def _fixed(c, llr, iters, algo=0):
    return O.decode(llr, c.N, c.punct["period"], T.puncture_matrix(c.punct), iters, c.perm, c.inv_perm, TAB,
                    algo=algo, want_lfinal=True)


def _es(c, llr, iters=I, algo=0):
    return R.decode_early_stop_batch(llr, c.N, c.punct, iters, c.perm, c.inv_perm, TAB, algo)


@pytest.fixture(scope="module")
def mixed48():
    """64 rows of N = 48 r = 1/3 valid-perm at 0 dB (seed fixed): mixed iteration counts."""
    c = M.DVBRCS2_Turbo(48, "1/3", I, interleaver="valid-perm")
    _, llr = R.bpsk_llrs(c, np.random.default_rng(48), 64, 0.0)
    return c, llr, _es(c, llr)


def test_helper_equals_fixed_decode_with_its_count(mixed48):
    c, llr, (bits, lf, nit) = mixed48
    for b in range(llr.shape[0]):
        rb, rl = _fixed(c, llr[b], int(nit[b]))
        assert np.array_equal(bits[b], rb), b
        np.testing.assert_array_equal(lf[b], rl)


@pytest.mark.parametrize("n,rate,interleaver,ebn0", [(212, "1/2", "valid-perm", 2.0), (48, "1/3", "reference", 4.0),
                                                     (212, "1/2", "reference", 4.0)])
def test_helper_equals_fixed_decode_other_configs(n, rate, interleaver, ebn0):
    c = M.DVBRCS2_Turbo(n, rate, I, interleaver=interleaver, inv_perm="stable")
    _, llr = R.bpsk_llrs(c, np.random.default_rng(n), 4, ebn0)
    llr[3] = 0.0   # an all-zero row: D_0 = D_1 = all 0, so it stops at 2
    bits, lf, nit = _es(c, llr)
    assert nit[3] == 2
    for b in range(4):
        rb, rl = _fixed(c, llr[b], int(nit[b]))
        assert np.array_equal(bits[b], rb)
        np.testing.assert_array_equal(lf[b], rl)


@pytest.mark.parametrize("iters", [1, 2])
def test_edge_counts(mixed48, iters):
    c, llr, _ = mixed48
    bits, lf, nit = _es(c, llr[:4], iters)
    assert (nit == iters).all()
    for b in range(4):
        rb, rl = _fixed(c, llr[b], iters)
        assert np.array_equal(bits[b], rb)
        np.testing.assert_array_equal(lf[b], rl)


def test_runs_to_the_cap_where_decisions_never_settle():
    """N = 212 r = 1/2 with the reference's non-bijective interleaver (stable
    inv_perm): the two decoders keep disagreeing, at every SNR."""
    c = M.DVBRCS2_Turbo(212, "1/2", I, inv_perm="stable")
    rng = np.random.default_rng(212)
    for ebn0 in (0.0, 2.0, 4.0, 6.0, 8.0):
        _, llr = R.bpsk_llrs(c, rng, 12, ebn0)
        assert (_es(c, llr)[2] == I).all(), ebn0


def test_mixed_counts_at_low_snr(mixed48):
    nit = mixed48[2][2]
    assert len(set(nit.tolist())) >= 3
    assert nit.min() <= 3
    assert (nit == I).any()
    assert nit.min() >= 2 and nit.max() <= I


def test_keyword_refuses_without_the_frame_decoder(monkeypatch):
    assert M.DVBRCS2_Turbo(48, "1/3", early_stop=True).early_stop
    assert not M.DVBRCS2_Turbo(48, "1/3").early_stop
    monkeypatch.setenv("TDEC_FRAME", "0")
    with pytest.raises(ValueError, match="frame decoder"):
        M.DVBRCS2_Turbo(48, "1/3", early_stop=True)
    with pytest.raises(ValueError, match="frame decoder"):
        M.DVB_RCS2_TurboCodec(block_length=48, code_rate="1/3", early_stop=True)
    with pytest.raises(ValueError, match="frame decoder"):
        M.turbo_decode(np.zeros(48 * 6, np.float32), 48, "1/3", early_stop=True)
    M.DVBRCS2_Turbo(48, "1/3")   # the default is untouched


def test_return_iters_needs_no_early_stop_keyword_to_exist():
    """The keyword surface exists without touching a device: signature only."""
    import inspect
    assert "return_iters" in inspect.signature(M.DVBRCS2_Turbo.decode_batch).parameters
    assert "n_iter" in inspect.signature(M.DVBRCS2_Turbo.decode_device).parameters
    assert "n_iter" in inspect.signature(M.DVBRCS2_Turbo.decode_planes_device).parameters
