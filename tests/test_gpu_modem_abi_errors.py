"""Argument refusals of the modem front end's C ABI (include/modem.h): mdm_map, mdm_demod,
mdm_fir, mdm_iq_quantize, mdm_iq_dequantize and their _dev forms, called through
_native.modem_lib().  Per bad argument: the return code, a substring of mdm_last_error(), and
that no output buffer (all pre-filled with 0x5A) was written.  Read off modem_api.hip: every
case is turned away by the library's own checks (or is a documented empty call) before a
kernel is launched -- the good arguments are small, so nothing here depends on that.

The order of the checks is part of what is pinned where a caller can observe it: the
demodulator's rule and bps, the FIR's shape and its taps pointer are looked at before the empty
call; the data pointers only after it, so an empty call with null buffers is MDM_OK.  One
refusal is made after the host form has staged its input: a complex128 table with bps 8, whose
size mdm_map looks at only then (mdm_map_dev looks at it at once, before the empty call)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulations_amd import _native as NT  # noqa: E402

EINVAL, OK = NT.TDEC_EINVAL, 0
FILL = 0x5A
IN, OUT, TAB, SCRATCH, CNT, STREAM = "in", "out", "tab", "scratch", "cnt", "stream"

# argument order of every entry point with a call that works (16 symbols or samples at the most)
MAP = dict(device=0, bits=IN, n_bits=24, bps=4, table=TAB, table_f64=0, syms=OUT)
DEMOD = dict(device=0, kind=3, syms=IN, sym_f64=0, n_sym=16, bps=4, labels=None, scale=3.0, cons=None, nan_raises=1,
             bits=OUT)
FIR = dict(device=0, x=IN, x_f64=0, n_x=16, taps=TAB, n_taps=4, up=1, down=1, offset=0, n_out=16, out=OUT)
QUANT = dict(device=0, sig=IN, sig_f64=0, n=16, iq=OUT)
DEQUANT = dict(device=0, raw=IN, n_pairs=16, sig=OUT)
GOOD = {
    "mdm_map": MAP, "mdm_map_dev": MAP | dict(stream=STREAM),
    "mdm_demod": DEMOD, "mdm_demod_dev": DEMOD | dict(nan_count=CNT, stream=STREAM),
    "mdm_fir": FIR, "mdm_fir_dev": FIR | dict(stream=STREAM),
    "mdm_iq_quantize": QUANT, "mdm_iq_quantize_dev": QUANT | dict(scratch=SCRATCH, stream=STREAM),
    "mdm_iq_dequantize": DEQUANT, "mdm_iq_dequantize_dev": DEQUANT | dict(stream=STREAM),
}


def _labels(n, i, v):
    lab = np.arange(n, dtype=np.int32)
    lab[i] = v
    return lab


_M, _Q, _F, _L = "bad mapper arguments", "QAM demod needs an even bps", "bad FIR arguments", "label table out of range"
_LONG, _NULL = "FIR too long for one call", "null buffer"
MAP_CASES = {
    "n_bits < 0": (dict(n_bits=-1), EINVAL, _M), "bps 0": (dict(bps=0), EINVAL, _M), "bps 9": (dict(bps=9), EINVAL, _M),
    "bps -1": (dict(bps=-1), EINVAL, _M), "null table": (dict(table=None), EINVAL, _M),
    "null table, n_bits 0": (dict(table=None, n_bits=0), EINVAL, _M),
    "complex128 table, bps 8": (dict(table_f64=1, bps=8), EINVAL, "complex128 mapper tables hold at most 128 points"),
    "null bits": (dict(bits=None), EINVAL, _NULL), "null syms": (dict(syms=None), EINVAL, _NULL),
    "n_bits 0, null buffers": (dict(n_bits=0, bits=None, syms=None), OK, ""),
}
DEMOD_CASES = {
    "n_sym < 0": (dict(n_sym=-1), EINVAL, "negative symbol count"),
    "GT0 bps 2": (dict(kind=0, bps=2), EINVAL, "GT0 demod has bps 1"),
    "QPSK bps 1": (dict(kind=1, bps=1), EINVAL, "QPSK demod has bps 2"),
    "PSK8 bps 2": (dict(kind=2, bps=2), EINVAL, "8PSK demod has bps 3"),
    "PSK8 bps 4": (dict(kind=2, bps=4), EINVAL, "8PSK demod has bps 3"),
    "QAM_AXIS bps 0": (dict(bps=0), EINVAL, _Q), "QAM_AXIS bps 3": (dict(bps=3), EINVAL, _Q),
    "QAM_AXIS bps 10": (dict(bps=10), EINVAL, _Q), "QAM_AXIS bps 16": (dict(bps=16), EINVAL, _Q),
    "QAM_AXIS bps 10, n_sym 0": (dict(bps=10, n_sym=0), EINVAL, _Q),
    "QAM_AXIS bps 18": (dict(bps=18), EINVAL, _Q),
    "PSK8 label -1": (dict(kind=2, bps=3, labels=_labels(8, 5, -1)), EINVAL, _L),
    "PSK8 label 8": (dict(kind=2, bps=3, labels=_labels(8, 7, 8)), EINVAL, _L),
    "QAM_AXIS label -1": (dict(labels=_labels(4, 0, -1)), EINVAL, _L),
    "QAM_AXIS label 4": (dict(labels=_labels(4, 3, 4)), EINVAL, _L),
    "QAM_AXIS label 4, n_sym 0": (dict(labels=_labels(4, 3, 4), n_sym=0), EINVAL, _L),
    "ARGMIN without cons": (dict(kind=4, bps=4, cons=None), EINVAL, "argmin demod needs a constellation"),
    "ARGMIN bps 7": (dict(kind=4, bps=7, cons=TAB), EINVAL, "argmin demod supports up to 64 points"),
    "ARGMIN bps 0": (dict(kind=4, bps=0, cons=TAB), EINVAL, "argmin demod supports up to 64 points"),
    "kind -1": (dict(kind=-1), EINVAL, "unknown demodulator kind"), "kind 5": (dict(kind=5), EINVAL, "unknown demodulator kind"),
    "kind 5, n_sym 0": (dict(kind=5, n_sym=0), EINVAL, "unknown demodulator kind"),
    "null syms": (dict(syms=None), EINVAL, _NULL), "null bits": (dict(bits=None), EINVAL, _NULL),
    "n_sym 0, null buffers": (dict(n_sym=0, syms=None, bits=None), OK, ""),
}
FIR_CASES = {
    "null taps": (dict(taps=None), EINVAL, "null taps"), "null taps, n_out 0": (dict(taps=None, n_out=0), EINVAL, "null taps"),
    "n_x 0": (dict(n_x=0), EINVAL, _F), "n_x < 0": (dict(n_x=-5), EINVAL, _F),
    "n_taps 0": (dict(n_taps=0), EINVAL, _F), "n_taps 257": (dict(n_taps=257), EINVAL, _F),
    "up 0": (dict(up=0), EINVAL, _F), "down 0": (dict(down=0), EINVAL, _F), "offset < 0": (dict(offset=-1), EINVAL, _F),
    "n_out < 0": (dict(n_out=-1), EINVAL, _F), "up 0, n_out 0": (dict(up=0, n_out=0), EINVAL, _F),
    "last output at 2^31": (dict(n_out=(1 << 31) - 3), EINVAL, _LONG),           # (n_out - 1) + 0 + 4 = 2^31
    "last output at 2^31 by down": (dict(n_out=(1 << 30) + 1, down=2), EINVAL, _LONG),
    "last output at 2^31 by offset": (dict(offset=(1 << 31) - 19), EINVAL, _LONG),
    "input at 2^31": (dict(n_x=(1 << 31) - 4), EINVAL, _LONG),                 # n_x * 1 + 4 = 2^31
    "input at 2^31 by up": (dict(n_x=1 << 28, up=8), EINVAL, _LONG),
    "input at 2^31, n_out 0": (dict(n_x=1 << 28, up=8, n_out=0), EINVAL, _LONG),
    "null x": (dict(x=None), EINVAL, _NULL), "null out": (dict(out=None), EINVAL, _NULL),
    "n_out 0, null buffers": (dict(n_out=0, x=None, out=None), OK, ""),
}
_Z = "zero-size array to reduction operation maximum"
QUANT_CASES = {"n 0": (dict(n=0), EINVAL, _Z), "n < 0": (dict(n=-1), EINVAL, _Z),
               "n 0, null buffers": (dict(n=0, sig=None, iq=None), EINVAL, _Z),
               "null sig": (dict(sig=None), EINVAL, _NULL), "null iq": (dict(iq=None), EINVAL, _NULL)}
DEQUANT_CASES = {"n_pairs < 0": (dict(n_pairs=-1), EINVAL, "negative sample count"),
                 "null raw": (dict(raw=None), EINVAL, _NULL), "null sig": (dict(sig=None), EINVAL, _NULL),
                 "n_pairs 0, null buffers": (dict(n_pairs=0, raw=None, sig=None), OK, "")}
CASES = {
    # the two forms look at a complex128 table's size at different moments: mdm_map_dev at once, mdm_map only
    # after staging, so that its empty call is MDM_OK and its null buffers are refused first
    "mdm_map": MAP_CASES | {
        "complex128 table, bps 8, n_bits 0": (dict(table_f64=1, bps=8, n_bits=0), OK, ""),
        "complex128 table, bps 8, null bits": (dict(table_f64=1, bps=8, bits=None), EINVAL, _NULL)},
    "mdm_map_dev": MAP_CASES | {
        "complex128 table, bps 8, n_bits 0": (dict(table_f64=1, bps=8, n_bits=0), EINVAL, "complex128 mapper tables"),
        "complex128 table, bps 8, null bits": (dict(table_f64=1, bps=8, bits=None), EINVAL, "complex128 mapper tables")},
    "mdm_demod": DEMOD_CASES, "mdm_demod_dev": DEMOD_CASES,
    "mdm_fir": FIR_CASES, "mdm_fir_dev": FIR_CASES,
    "mdm_iq_quantize": QUANT_CASES,
    "mdm_iq_quantize_dev": QUANT_CASES | {"null scratch": (dict(scratch=None), EINVAL, _NULL)},
    "mdm_iq_dequantize": DEQUANT_CASES, "mdm_iq_dequantize_dev": DEQUANT_CASES,
}
PARAMS = [(name, case) for name in CASES for case in CASES[name]]


@pytest.fixture(scope="module")
def env():
    """Inputs of zeros, a table of zeros (labels, taps, constellation alike), and outputs,
    scratch and NaN counter filled with 0x5A on both sides."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = {"h_in": np.zeros(4096, np.uint8), "tab": np.zeros(512, np.float64), "h_out": np.full(1 << 16, FILL, np.uint8),
         "d_in": torch.zeros(4096, dtype=torch.uint8, device="cuda")}
    for k, n in (("d_out", 1 << 16), ("d_scratch", 8), ("d_cnt", 4)):
        e[k] = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    yield e
    _untouched(e)


def _untouched(e):
    torch.cuda.synchronize()
    assert (e["h_out"] == FILL).all()
    for k in ("d_out", "d_scratch", "d_cnt"):
        assert bool((e[k] == FILL).all()), k


def _call(e, name, change):
    devf = name.endswith("_dev")
    where = {IN: e["d_in"] if devf else e["h_in"], OUT: e["d_out"] if devf else e["h_out"], TAB: e["tab"],
             SCRATCH: e["d_scratch"], CNT: e["d_cnt"]}
    a = dict(GOOD[name])
    assert set(change) <= set(a), (name, change)
    a.update(change)
    keep, args = [], []
    for v in a.values():
        if isinstance(v, str):
            v = C.c_void_p(torch.cuda.current_stream().cuda_stream) if v == STREAM else NT.ptr(where[v])
        elif isinstance(v, np.ndarray):
            keep.append(v)
            v = NT.ptr(v)
        args.append(v)
    return getattr(NT.modem_lib(), name)(*args)


def test_the_table_covers_the_ten_entry_points():
    front = [n for n in NT.MODEM_EXPORTS if n.split("_dev")[0] in
             ("mdm_map", "mdm_demod", "mdm_fir", "mdm_iq_quantize", "mdm_iq_dequantize")]
    assert sorted(front) == sorted(CASES) == sorted(GOOD) and len(front) == 10


@pytest.mark.parametrize("name,case", PARAMS)
def test_refusal(env, name, case):
    change, rc, msg = CASES[name][case]
    L = NT.modem_lib()
    assert _call(env, name, change) == rc, L.mdm_last_error().decode()
    if rc:
        err = L.mdm_last_error().decode()
        assert err and msg in err
    _untouched(env)
