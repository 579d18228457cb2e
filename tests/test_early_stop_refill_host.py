"""Host side of es_decoder="refill" (DESIGN.md §8.3): the option, the BER tool's
argument and resume key, the C ABI's names, and the refill schedule model that the
GPU tests compare tdec_es_refill_stats with.  No device is touched."""
import argparse
import os
import re

import numpy as np
import pytest

from modulations_amd import _native, ber
from modulations_amd import dvb_rcs2_turbo as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdec_reserve_es_refill", "tdec_decode_planes_es_refill_dev", "tdec_decode_batch_es_refill_dev",
         "tdec_decode_batch_es_refill", "tdec_es_refill_stats")


def refill_schedule(n_iter, waves=1):
    """(trips, refills) of one persistent wave over rows with these iteration counts,
    by the order include/tdec.h documents: at the top of every trip the free lanes (a
    lane whose codeword has ended, or that never had one) take the next rows of the
    batch in ascending lane order; a trip runs one iteration of every lane; a lane
    whose codeword has run its n_iter iterations is free from the next trip on.  The
    wave stops when no row is left and no lane decodes."""
    assert waves == 1
    n_iter = np.asarray(n_iter, np.int64)
    assert n_iter.ndim == 1 and (n_iter >= 1).all()
    left = np.zeros(64, np.int64)        # iterations each lane's codeword still has to run (0: free)
    nxt = trips = refills = 0
    while True:
        for lane in np.flatnonzero(left == 0):   # ascending
            if nxt == len(n_iter):
                break
            left[lane] = n_iter[nxt]
            nxt += 1
            refills += 1
        if not left.any():
            return trips, refills
        trips += 1
        left[left > 0] -= 1


def test_refill_schedule_by_hand():
    # 64 rows of 2 fill the wave and end together after 2 trips; the 64 rows of 3 then take 3 more
    assert refill_schedule([2] * 64 + [3] * 64) == (5, 128)
    # one row of 8 among 127 of 2, in the first 64: the other 63 lanes turn over once (trips 1-2 and 3-4)
    # inside the 8 trips the long row needs; whole tiles would run 8 + 2
    for at in (0, 17, 63):
        v = [2] * 127
        v.insert(at, 8)
        assert refill_schedule(v) == (8, 128), at
    # the same row handed out at the first refill (trip 3) ends on trip 10
    assert refill_schedule([2] * 127 + [8]) == (10, 128)
    assert refill_schedule([]) == (0, 0)
    assert refill_schedule([1]) == (1, 1)
    assert refill_schedule([3] + [1] * 64) == (3, 65)   # lanes 1-63 turn over while lane 0 decodes


def test_refill_schedule_bounds():
    rng = np.random.default_rng(3)
    for B in (1, 64, 65, 200, 320):
        n = rng.integers(2, 9, B)
        trips, refills = refill_schedule(n)
        assert refills == B
        tile_trips = sum(int(n[i:i + 64].max()) for i in range(0, B, 64))
        assert -(-int(n.sum()) // 64) <= trips <= tile_trips
        assert trips >= int(n.max())


def test_refill_codec_constructs_without_a_device(monkeypatch):
    for n in sorted(M.INTERLEAVER_PARAMS):
        c = M.DVBRCS2_Turbo(n, "1/3", early_stop=True, es_decoder="refill")
        assert c.early_stop and c.es_decoder == "refill" and c._h is None
    monkeypatch.setenv("TDEC_FRAME", "0")
    c = M.DVBRCS2_Turbo(848, "1/3", early_stop=True, es_decoder="refill")
    assert c.es_decoder == "refill" and c._h is None
    c = M.DVB_RCS2_TurboCodec(48, "1/3", early_stop=True, es_decoder="refill")
    assert c.es_decoder == "refill" and c._h is None
    assert callable(c.refill_stats)


def test_default_is_still_the_frame_decoder():
    assert M.DVBRCS2_Turbo(48, "1/3").es_decoder == "frame"
    assert M.DVBRCS2_Turbo(48, "1/3", early_stop=True).es_decoder == "frame"
    assert M.DVBRCS2_Turbo(48, "1/3", es_decoder="refill").early_stop is False   # ignored without early_stop


@pytest.mark.parametrize("bad", ["auto", "Refill", "refil", "", None, 1, ("refill",)])
def test_other_values_are_refused(bad):
    with pytest.raises(ValueError, match="es_decoder"):
        M.DVBRCS2_Turbo(48, "1/3", early_stop=True, es_decoder=bad)
    with pytest.raises(ValueError, match="es_decoder"):
        M.DVBRCS2_Turbo(48, "1/3", es_decoder=bad)


def test_ber_argument():
    ap = ber.arg_parser()
    assert ap.parse_args([]).es_decoder == "frame"
    assert ap.parse_args(["--early-stop", "--es-decoder", "refill"]).es_decoder == "refill"
    with pytest.raises(SystemExit):
        ap.parse_args(["--es-decoder", "auto"])


def test_ber_resume_key(tmp_path):
    def ns(**kw):
        d = dict(mod="QPSK", n=48, rate="1/3", algo="max-log", iterations=8, interleaver="valid-perm",
                 codewords=192, seed=5, early_stop=False, es_decoder="frame")
        d.update(kw)
        return argparse.Namespace(**d)
    plain, frame = ber.sweep_config(ns()), ber.sweep_config(ns(early_stop=True))
    tile = ber.sweep_config(ns(early_stop=True, es_decoder="tile"))
    refill = ber.sweep_config(ns(early_stop=True, es_decoder="refill"))
    assert "es_decoder" not in plain and "es_decoder" not in frame   # the default still adds no key
    assert refill == {**frame, "es_decoder": "refill"}
    assert ber.sweep_config(ns(es_decoder="refill")) == plain   # without --early-stop the option does nothing
    path = str(tmp_path / "sweep.json")
    ber.save_results(path, refill, [{"ebn0_db": 1.0}])
    assert list(ber.load_resume(path, refill)) == [1.0]
    for other in (frame, tile, plain):
        with pytest.raises(ValueError, match="another sweep"):
            ber.load_resume(path, other)
    ber.save_results(path, tile, [{"ebn0_db": 1.0}])
    with pytest.raises(ValueError, match="another sweep"):
        ber.load_resume(path, refill)


def test_abi_names():
    src = open(os.path.join(ROOT, "include", "tdec.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTS
        assert re.search(rf"^int {name}\(", src, re.M), name
    assert "ascending" in src and "lane order" in src   # the refill order is part of the documented interface
