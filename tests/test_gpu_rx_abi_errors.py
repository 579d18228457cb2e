"""Argument refusals of the burst-receive chain's C ABI (include/modem.h): mdm_mix,
mdm_burst_find, mdm_xcorr_peak, mdm_carrier and their _dev forms, called through
_native.modem_lib(), in the manner of tests/test_gpu_modem_abi_errors.py.  Per bad argument: the
return code, a substring of mdm_last_error(), and that no output buffer (all pre-filled with
0x5A) was written.  Read off modem_api.hip: every refusal is made by the library's own checks
before anything is allocated or launched, the "too long" ones included, so the sizes named here
are never touched.

Three calls are accepted.  An empty mixer call (n = 0) and an empty carrier batch (n_cand = 0)
return 0 with null buffers and write nothing.  A carrier call without symbols (n = 0) accepts
null syms / out and writes only the final state, which is the initial phase and frequency."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulations_amd import _native as NT  # noqa: E402

EINVAL, OK = NT.TDEC_EINVAL, 0
FILL = 0x5A
IN, OUT, OUT2, FIN, TAB, SCRATCH, STREAM = "in", "out", "out2", "fin", "tab", "scratch", "stream"
PAR = "par"      # the carrier's per-stream parameters: host memory for mdm_carrier, device memory for mdm_carrier_dev

# argument order of every entry point with a call that works
MIX = dict(device=0, sig=IN, sig_f64=0, n=16, i0=0, dc=None, w=0.0, fs=1.0, out=OUT)
BURST = dict(device=0, sig=IN, sig_f64=0, n=2048, dc=None, win=16, preamble_len=8)
XCORR = dict(device=0, region=IN, n_region=64, w=PAR, n_w=8, corr=None)
CARRIER = dict(device=0, syms=IN, n_cand=2, n=8, phase=PAR, freq=PAR, alpha=PAR, kind=PAR, out=OUT, final=FIN)
GOOD = {
    "mdm_mix": MIX, "mdm_mix_dev": MIX | dict(stream=STREAM),
    "mdm_burst_find": BURST | dict(burst_start=OUT, max_power=OUT2, smooth=None),
    "mdm_burst_find_dev": BURST | dict(smooth=None, result=OUT, scratch=SCRATCH, stream=STREAM),
    "mdm_xcorr_peak": XCORR | dict(argmax=OUT, peak=OUT2),
    "mdm_xcorr_peak_dev": XCORR | dict(result=OUT, scratch=SCRATCH, stream=STREAM),
    "mdm_carrier": CARRIER, "mdm_carrier_dev": CARRIER | dict(stream=STREAM),
}

_NULL = "null buffer"
_WIN, _SHORT = "smoothing window must be 1..1024 samples", "capture shorter than the smoothing window"
_TAPS, _REGION = "sync waveform must have 1..1024 taps", "search region shorter than the sync waveform"
_NEG = "negative carrier batch or length"
MIX_CASES = {
    "n < 0": (dict(n=-1), EINVAL, "negative sample count"),
    "null sig": (dict(sig=None), EINVAL, _NULL), "null out": (dict(out=None), EINVAL, _NULL),
    "n 0": (dict(n=0), OK, ""), "n 0, null buffers": (dict(n=0, sig=None, out=None), OK, ""),
}
BURST_CASES = {
    "win 0": (dict(win=0), EINVAL, _WIN), "win -1": (dict(win=-1), EINVAL, _WIN), "win 1025": (dict(win=1025), EINVAL, _WIN),
    "win 1025, long capture": (dict(win=1025, n=4096), EINVAL, _WIN),
    "n < win": (dict(n=15), EINVAL, _SHORT), "n 0": (dict(n=0), EINVAL, _SHORT), "n < 0": (dict(n=-1), EINVAL, _SHORT),
    "n 1023, win 1024": (dict(n=1023, win=1024), EINVAL, _SHORT),
    "preamble_len < 0": (dict(preamble_len=-1), EINVAL, "negative preamble length"),
    "2^31 tiles": (dict(n=(1 << 41) - 1023), EINVAL, "capture too long"),       # ceil(n / 1024) = 2^31
    "null sig": (dict(sig=None), EINVAL, _NULL),
}
XCORR_CASES = {
    "n_w 0": (dict(n_w=0), EINVAL, _TAPS), "n_w -1": (dict(n_w=-1), EINVAL, _TAPS),
    "n_w 1025": (dict(n_w=1025, n_region=4096), EINVAL, _TAPS),
    "n_region < n_w": (dict(n_region=7), EINVAL, _REGION), "n_region 0": (dict(n_region=0), EINVAL, _REGION),
    "n_region < 0": (dict(n_region=-1), EINVAL, _REGION),
    "n_region 1023, n_w 1024": (dict(n_region=1023, n_w=1024), EINVAL, _REGION),
    "2^31 workgroups": (dict(n_region=(1 << 41) - 1016), EINVAL, "search region too long"),   # ceil(n_out / 1024) = 2^31
    "null region": (dict(region=None), EINVAL, _NULL), "null w": (dict(w=None), EINVAL, _NULL),
}
CARRIER_CASES = {
    "n_cand < 0": (dict(n_cand=-1), EINVAL, _NEG), "n < 0": (dict(n=-1), EINVAL, _NEG),
    "n_cand < 0, n 0": (dict(n_cand=-1, n=0), EINVAL, _NEG),
    "null phase": (dict(phase=None), EINVAL, _NULL), "null freq": (dict(freq=None), EINVAL, _NULL),
    "null alpha": (dict(alpha=None), EINVAL, _NULL), "null kind": (dict(kind=None), EINVAL, _NULL),
    "null final": (dict(final=None), EINVAL, _NULL), "null final, n 0": (dict(final=None, n=0), EINVAL, _NULL),
    "null syms": (dict(syms=None), EINVAL, _NULL), "null out": (dict(out=None), EINVAL, _NULL),
    "n_cand 0": (dict(n_cand=0), OK, ""),
    "n_cand 0, null buffers": (dict(n_cand=0, syms=None, phase=None, freq=None, alpha=None, kind=None, out=None,
                                    final=None), OK, ""),
    "n 0, null syms and out": (dict(n=0, syms=None, out=None), OK, "final"),
}
CASES = {
    "mdm_mix": MIX_CASES, "mdm_mix_dev": MIX_CASES,
    "mdm_burst_find": BURST_CASES | {"null burst_start": (dict(burst_start=None), EINVAL, _NULL)},
    "mdm_burst_find_dev": BURST_CASES | {"null result": (dict(result=None), EINVAL, _NULL),
                                         "null scratch": (dict(scratch=None), EINVAL, _NULL)},
    "mdm_xcorr_peak": XCORR_CASES | {"null argmax": (dict(argmax=None), EINVAL, _NULL)},
    "mdm_xcorr_peak_dev": XCORR_CASES | {"null result": (dict(result=None), EINVAL, _NULL),
                                         "null scratch": (dict(scratch=None), EINVAL, _NULL)},
    "mdm_carrier": CARRIER_CASES | {
        "kind 3": (dict(kind=np.array([0, 3], np.int32)), EINVAL, "unknown carrier detector kind"),
        "kind -1": (dict(kind=np.array([-1, 0], np.int32)), EINVAL, "unknown carrier detector kind"),
        "kind 3, n 0": (dict(kind=np.array([2, 3], np.int32), n=0), EINVAL, "unknown carrier detector kind"),
        # the kinds are read after the pointers are checked, and not at all for an empty batch
        "kind 3, null final": (dict(kind=np.array([0, 3], np.int32), final=None), EINVAL, _NULL),
        "kind 3, n_cand 0": (dict(kind=np.array([0, 3], np.int32), n_cand=0), OK, "")},
    "mdm_carrier_dev": CARRIER_CASES,
}
PARAMS = [(name, case) for name in CASES for case in CASES[name]]


@pytest.fixture(scope="module")
def env():
    """Inputs and parameters of zeros (so every carrier kind is 0 and every initial state 0) on
    both sides; outputs, scratch and the carrier's final state filled with 0x5A on both sides."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = {"h_in": np.zeros(1 << 16, np.uint8), "h_par": np.zeros(4096, np.float64),
         "d_in": torch.zeros(1 << 16, dtype=torch.uint8, device="cuda"),
         "d_par": torch.zeros(4096, dtype=torch.float64, device="cuda")}
    for k in ("out", "out2", "fin"):
        e["h_" + k] = np.full(1 << 12, FILL, np.uint8)
    for k in ("d_out", "d_out2", "d_fin", "d_scratch"):
        e[k] = torch.full((1 << 12,), FILL, dtype=torch.uint8, device="cuda")
    yield e
    _untouched(e)


def _untouched(e, but=()):
    torch.cuda.synchronize()
    for k in ("h_out", "h_out2", "h_fin"):
        assert k in but or (e[k] == FILL).all(), k
    for k in ("d_out", "d_out2", "d_fin", "d_scratch"):
        assert k in but or bool((e[k] == FILL).all()), k


def _call(e, name, change):
    devf = name.endswith("_dev")
    side = "d_" if devf else "h_"
    where = {IN: e[side + "in"], PAR: e[side + "par"], OUT: e[side + "out"], OUT2: e[side + "out2"], FIN: e[side + "fin"],
             SCRATCH: e["d_scratch"]}
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


def test_the_table_covers_the_eight_entry_points():
    rx = [n for n in NT.MODEM_EXPORTS if n.split("_dev")[0] in
          ("mdm_mix", "mdm_burst_find", "mdm_xcorr_peak", "mdm_carrier")]
    assert sorted(rx) == sorted(CASES) == sorted(GOOD) and len(rx) == 8
    for name, good in GOOD.items():          # the argument lists are the declared ones
        assert len(good) == len(getattr(NT.modem_lib(), name).argtypes), name


@pytest.mark.parametrize("name,case", PARAMS)
def test_refusal(env, name, case):
    change, rc, msg = CASES[name][case]
    L = NT.modem_lib()
    assert _call(env, name, change) == rc, L.mdm_last_error().decode()
    if rc:
        err = L.mdm_last_error().decode()
        assert err and msg in err
        _untouched(env)
    elif msg == "final":
        # no symbols: the final state is the initial one (phase, freq = 0, 0 per stream), nothing else is written
        key = "d_fin" if name.endswith("_dev") else "h_fin"
        _untouched(env, but=(key,))
        fin = env[key].cpu().numpy() if name.endswith("_dev") else env[key]
        assert not fin[:32].any() and (fin[32:] == FILL).all()
        env[key][:32] = FILL
    else:
        _untouched(env)
