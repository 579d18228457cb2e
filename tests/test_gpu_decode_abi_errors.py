"""Argument checks of the nine decode entry points (include/tdec.h: tdec_decode_planes*_dev,
tdec_decode_batch*_dev, tdec_decode_batch*), through the C ABI: the return code of every
rejected call, the order in which an entry point looks at its arguments where a caller can
observe it, and that a rejected call says why (tdec_last_error) and writes nothing.  No call
here reaches a kernel with a bad pointer: each is turned away by the library's own checks."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulations_amd import _native as NT  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402

PLANES_DEV = ("tdec_decode_planes_dev", "tdec_decode_planes_es_dev", "tdec_decode_planes_es_tile_dev")
BATCH_DEV = ("tdec_decode_batch_dev", "tdec_decode_batch_es_dev", "tdec_decode_batch_es_tile_dev")
HOST = ("tdec_decode_batch", "tdec_decode_batch_es", "tdec_decode_batch_es_tile")
ALL = PLANES_DEV + BATCH_DEV + HOST
ES_FRAME = ("tdec_decode_planes_es_dev", "tdec_decode_batch_es_dev", "tdec_decode_batch_es")
RESERVED = 64


@pytest.fixture(scope="module")
def env():
    """One N = 48 r = 1/3 handle reserved for 64 codewords, and valid buffers for 65 rows:
    device LLR rows and planes, host LLR rows, and outputs filled with 7 on both sides."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = M.DVBRCS2_Turbo(48, "1/3")
    c.reserve(RESERVED)
    B, n = RESERVED + 1, c.handle.llr_len
    e = {"c": c, "h": c.handle.h, "n": n, "B": B,
         "d_llr": torch.zeros((B, n), dtype=torch.float32, device="cuda"),
         "d_planes": torch.zeros(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda"),
         "d_bits": torch.full((B, c.k_info), 7, dtype=torch.int32, device="cuda"),
         "d_lf": torch.full((B, c.k_info), 7.0, dtype=torch.float64, device="cuda"),
         "d_nit": torch.full((B,), 7, dtype=torch.int32, device="cuda"),
         "llr": np.zeros((B, n), np.float32),
         "bits": np.full((B, c.k_info), 7, np.int32),
         "lf": np.full((B, c.k_info), 7.0),
         "nit": np.full(B, 7, np.int32)}
    yield e
    torch.cuda.synchronize()
    assert (e["d_bits"] == 7).all() and (e["d_lf"] == 7.0).all() and (e["d_nit"] == 7).all()
    assert (e["bits"] == 7).all() and (e["lf"] == 7.0).all() and (e["nit"] == 7).all()


def _call(e, name, B, *, h="handle", inp="valid", bits="valid", stride=None):
    """name(h, B, input[, stride], bits, lfinal[, n_iter][, stream]) with valid or null
    pointers; returns the code, and checks that a failure left a message."""
    host = name in HOST
    h = e["h"] if h == "handle" else None
    if inp == "valid":
        inp = NT.ptr(e["llr"] if host else e["d_planes"] if name in PLANES_DEV else e["d_llr"])
    else:
        inp = None
    valid_out = bits == "valid"
    args = [h, B, inp]
    if name not in PLANES_DEV:
        args.append(e["n"] if stride is None else stride)
    args += [NT.ptr(e["bits" if host else "d_bits"]) if valid_out else None,
             NT.ptr(e["lf" if host else "d_lf"]) if valid_out else None]
    if "_es" in name:
        args.append(NT.ptr(e["nit" if host else "d_nit"]) if valid_out else None)
    if not host:
        args.append(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = getattr(NT.lib(), name)(*args)
    if rc != 0:
        assert NT.lib().tdec_last_error(), name
    return rc


@pytest.mark.parametrize("name", ALL)
def test_null_handle_and_negative_batch(env, name):
    assert _call(env, name, 1, h=None) == NT.TDEC_EINVAL
    assert _call(env, name, 0, h=None) == NT.TDEC_EINVAL
    assert _call(env, name, -1) == NT.TDEC_EINVAL
    assert _call(env, name, -1, inp=None, bits=None) == NT.TDEC_EINVAL


@pytest.mark.parametrize("name", ALL)
def test_empty_batch_is_a_no_op_with_null_pointers(env, name):
    assert _call(env, name, 0, inp=None, bits=None) == 0


@pytest.mark.parametrize("name", HOST)
def test_host_forms_check_the_stride_before_the_empty_batch(env, name):
    assert _call(env, name, 0, inp=None, bits=None, stride=env["n"] - 1) == NT.TDEC_ESHORT
    assert _call(env, name, 0, stride=env["n"] - 1) == NT.TDEC_ESHORT


@pytest.mark.parametrize("name", BATCH_DEV)
def test_dev_forms_pass_an_empty_batch_before_the_stride(env, name):
    assert _call(env, name, 0, inp=None, bits=None, stride=env["n"] - 1) == 0


@pytest.mark.parametrize("name", ALL)
def test_null_data_pointers(env, name):
    assert _call(env, name, 1, inp=None) == NT.TDEC_EINVAL
    assert _call(env, name, 1, bits=None) == NT.TDEC_EINVAL


@pytest.mark.parametrize("name", BATCH_DEV + HOST)
def test_short_rows(env, name):
    assert _call(env, name, 1, stride=env["n"] - 1) == NT.TDEC_ESHORT
    assert _call(env, name, 1, stride=0) == NT.TDEC_ESHORT


def test_capacity_comes_before_the_pointers_on_the_plain_batch_form(env):
    B = env["B"]
    assert _call(env, "tdec_decode_batch_dev", B) == NT.TDEC_ECAPACITY
    assert _call(env, "tdec_decode_batch_dev", B, inp=None, bits=None) == NT.TDEC_ECAPACITY
    torch.cuda.synchronize()
    assert (env["d_bits"] == 7).all() and (env["d_lf"] == 7.0).all()


def test_capacity_on_the_early_stop_tile_batch_form(env):
    """Above the reservation with valid pointers: TDEC_ECAPACITY, nothing written.  This
    entry point looks at its pointers first, so with null pointers the same call is
    TDEC_EINVAL (tdec_decode_batch_dev answers TDEC_ECAPACITY there, above)."""
    B = env["B"]
    assert _call(env, "tdec_decode_batch_es_tile_dev", B) == NT.TDEC_ECAPACITY
    assert _call(env, "tdec_decode_batch_es_tile_dev", B, inp=None, bits=None) == NT.TDEC_EINVAL
    torch.cuda.synchronize()
    assert (env["d_bits"] == 7).all() and (env["d_lf"] == 7.0).all() and (env["d_nit"] == 7).all()


@pytest.mark.parametrize("name", ES_FRAME)
def test_unavailable_frame_decoder_comes_after_the_pointers(env, name, monkeypatch):
    monkeypatch.setenv("TDEC_FRAME", "0")
    assert _call(env, name, 1) == NT.TDEC_EUNSUPPORTED
    assert b"TDEC_FRAME" in NT.lib().tdec_last_error()
    assert _call(env, name, 1, bits=None) == NT.TDEC_EINVAL
    assert _call(env, name, 1, inp=None) == NT.TDEC_EINVAL
    assert _call(env, name, 0, inp=None, bits=None) == 0
    if name != "tdec_decode_planes_es_dev":   # the stride check comes before it too
        assert _call(env, name, 1, stride=env["n"] - 1) == NT.TDEC_ESHORT
