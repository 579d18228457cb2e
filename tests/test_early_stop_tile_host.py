"""Host side of es_decoder="tile" (DESIGN.md §8.1): the option, the BER tool's
argument and resume key, and the C ABI's names.  No device is touched."""
import argparse
import os
import re

import pytest

from modulations_amd import _native, ber
from modulations_amd import dvb_rcs2_turbo as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdec_decode_batch_es_tile", "tdec_decode_planes_es_tile_dev", "tdec_decode_batch_es_tile_dev")


def test_tile_codec_constructs_without_a_device(monkeypatch):
    c = M.DVBRCS2_Turbo(848, "1/3", early_stop=True, es_decoder="tile")   # beyond the frame decoder's blocks
    assert c.early_stop and c.es_decoder == "tile" and c._h is None
    monkeypatch.setenv("TDEC_FRAME", "0")
    c = M.DVB_RCS2_TurboCodec(48, "1/3", early_stop=True, es_decoder="tile")
    assert c.es_decoder == "tile" and c._h is None
    with pytest.raises(ValueError, match="frame decoder"):
        M.DVBRCS2_Turbo(48, "1/3", early_stop=True)


def test_default_is_the_frame_decoder():
    assert M.DVBRCS2_Turbo(48, "1/3").es_decoder == "frame"
    assert M.DVBRCS2_Turbo(48, "1/3", early_stop=True).es_decoder == "frame"
    assert M.DVBRCS2_Turbo(48, "1/3", es_decoder="tile").early_stop is False   # ignored without early_stop


@pytest.mark.parametrize("bad", ["auto", "Tile", "", None, 1])
def test_bad_value_is_refused(bad):
    with pytest.raises(ValueError, match="es_decoder"):
        M.DVBRCS2_Turbo(48, "1/3", early_stop=True, es_decoder=bad)
    with pytest.raises(ValueError, match="es_decoder"):
        M.DVBRCS2_Turbo(48, "1/3", es_decoder=bad)


def test_ber_argument():
    ap = ber.arg_parser()
    assert ap.parse_args([]).es_decoder == "frame"
    assert ap.parse_args(["--early-stop", "--es-decoder", "tile"]).es_decoder == "tile"
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
    # the default adds no key: files of earlier sweeps keep resuming
    assert "es_decoder" not in plain and "es_decoder" not in frame
    assert frame == ber.sweep_config(argparse.Namespace(**{k: v for k, v in vars(ns(early_stop=True)).items()
                                                           if k != "es_decoder"}))
    assert tile == {**frame, "es_decoder": "tile"}
    assert ber.sweep_config(ns(es_decoder="tile")) == plain   # without --early-stop the option does nothing
    path = str(tmp_path / "sweep.json")
    ber.save_results(path, tile, [{"ebn0_db": 1.0}])
    assert list(ber.load_resume(path, tile)) == [1.0]
    with pytest.raises(ValueError, match="another sweep"):
        ber.load_resume(path, frame)
    ber.save_results(path, frame, [{"ebn0_db": 1.0}])
    with pytest.raises(ValueError, match="another sweep"):
        ber.load_resume(path, tile)


def test_abi_names():
    src = open(os.path.join(ROOT, "include", "tdec.h")).read()
    for name in NAMES:
        assert name in _native.EXPORTS
        assert re.search(rf"^int {name}\(", src, re.M), name
