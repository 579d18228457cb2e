"""Argument refusals of the workload generators' C ABI (include/tdec.h): the cases of
tdec_workload_dev, tdec_info_bits_dev, tdec_encode_dev, tdec_workload_fading_dev,
tdec_workload_branches_dev, tdec_workload_frame_dev, tdec_workload_frame_branches_dev and
tdec_count_errors_dev, as
(return code, substring of tdec_last_error()) per bad argument, for the GPU test file that owns
each call.  Every case is refused (or is an empty batch) before anything is launched.

The order of the checks is part of what is pinned: a bad handle, B or cw0 (and, in the branch
calls, R) is refused even when B == 0; B == 0 returns 0 whatever the pointers; the N % 4
refusal comes after every other one, and N = 1028 (a multiple of 4 the staged encoder does not hold)
is refused in the same place."""
import numpy as np

from modulations_amd import _native as N
from modulations_amd import demap as D
from modulations_amd import dvb_rcs2_turbo as M
from modulations_amd import tables as T

EINVAL = N.TDEC_EINVAL
B, R, S = 3, 2, 8                                         # the framing calls' batch; plen = 2, dlen = 7
_KEEP = {}


def _env():
    """Handles (N = 48, N = 50: no multiple of 4, and N = 1028: above the staged encoder's 1024) and
    device buffers, made once."""
    import torch
    if not _KEEP:
        c = M.DVBRCS2_Turbo(48, "1/3")
        perm = ((7 * np.arange(50) + 3) % 50).astype(np.int32)
        tables = T.packed_tables(c.next_state, c.out_W, c.out_Y, c.prev_state, c.prev_input)
        odd = M._Handle(0, 50, T.PUNCTURE_PATTERNS["1/3"], 8, 0, perm, np.argsort(perm).astype(np.int32), tables)
        pbig = ((7 * np.arange(1028) + 3) % 1028).astype(np.int32)
        big = M._Handle(0, 1028, T.PUNCTURE_PATTERNS["1/3"], 8, 0, pbig, np.argsort(pbig).astype(np.int32), tables)
        tab = np.ascontiguousarray(D.constellation("16QAM").astype(np.complex64)).view(np.float32)
        buf = torch.full((B * R * 1024,), np.nan, dtype=torch.complex64, device="cuda")   # any output fits
        _KEEP.update(c=c, h=c.handle.h, odd=odd, big=big, tab=tab, buf=buf, p=N.ptr(buf), t=N.ptr(tab))
    return _KEEP


def _good(name):
    e = _env()
    h, p, t = e["h"], e["p"], e["t"]
    return {
        "tdec_workload_dev": [h, B, 0, 1, t, 16, 4, 0.1, p, p, None],
        "tdec_info_bits_dev": [h, B, 0, 1, p, None],
        "tdec_encode_dev": [h, B, p, p, None],
        "tdec_workload_fading_dev": [h, B, 0, 1, t, 16, 4, 0.1, 0.0, 1, p, p, p, None],
        "tdec_workload_branches_dev": [h, B, R, 0, 1, t, 16, 4, 0.1, 0.0, 1, p, p, p, None],
        "tdec_workload_frame_dev": [0, p, p, B, S, 1, 2, 7, p, 0.1, 0, 1, 0.0, p, None, None],
        "tdec_workload_frame_branches_dev": [0, p, p, B, R, S, 1, 2, 7, p, 0.1, 0, 1, 0.0, p, None, None],
        "tdec_count_errors_dev": [h, B, 0, 1, p, p, None],
    }[name]


def _symbol_cases(o, head, body):
    """The symbol generators: o = 0, or 1 where R stands behind B; head / body: their two wordings."""
    return {
        "null handle": ({0: None}, EINVAL, head), "B < 0": ({1: -1}, EINVAL, head),
        "cw0 < 0": ({2 + o: -1}, EINVAL, head),
        "null handle, B == 0": ({0: None, 1: 0}, EINVAL, head), "cw0 < 0, B == 0": ({1: 0, 2 + o: -1}, EINVAL, head),
        "null table": ({4 + o: None}, EINVAL, body), "M != 1 << bps": ({5 + o: 8}, EINVAL, body),
        "bps 0": ({6 + o: 0}, EINVAL, body), "bps 9": ({5 + o: 512, 6 + o: 9}, EINVAL, body),
        "sigma < 0": ({7 + o: -0.1}, EINVAL, body), "sigma NaN": ({7 + o: np.nan}, EINVAL, body),
        "N % 4": ({0: "odd"}, EINVAL, "N % 4 == 0"), "N % 4 comes last": ({0: "odd", 4 + o: None}, EINVAL, body),
        "N = 1028": ({0: "big"}, EINVAL, "N <= 1024"), "N = 1028 comes last": ({0: "big", 4 + o: None}, EINVAL, body),
    }


def _fade_cases(o, body):
    """K, coh, gains and symbols of the fading forms (K at 8 + o)."""
    return {"K < 0": ({8 + o: -1.0}, EINVAL, body), "K inf": ({8 + o: np.inf}, EINVAL, body),
            "K NaN": ({8 + o: np.nan}, EINVAL, body), "coh < 1": ({9 + o: 0}, EINVAL, body),
            "null symbols": ({10 + o: None}, EINVAL, body), "null gains": ({11 + o: None}, EINVAL, body),
            "B == 0, null pointers": ({1: 0, 4 + o: None, 10 + o: None, 11 + o: None, 12 + o: None}, 0, "")}


def _frame_cases(o, head, long_):
    """The framing calls: o = 0, or 1 where R stands behind B."""
    body = "S, coh, plen, dlen >= 1"
    big = 1 << 30
    cases = {"B < 0": ({3: -1}, EINVAL, head), "cw0 < 0": ({10 + o: -1}, EINVAL, head),
             "cw0 < 0, B == 0": ({3: 0, 10 + o: -1}, EINVAL, head),
             "B == 0, null pointers": ({1: None, 2: None, 3: 0, 8 + o: None, 13 + o: None}, 0, ""),
             "T > INT32_MAX": ({4 + o: big, 6 + o: 1, 7 + o: 1}, EINVAL, long_)}
    for what, i in (("y", 1), ("gains", 2), ("pilots", 8 + o), ("frames", 13 + o)):
        cases[f"null {what}"] = ({i: None}, EINVAL, body)
    for what, i in (("S", 4 + o), ("coh", 5 + o), ("plen", 6 + o), ("dlen", 7 + o)):
        cases[f"{what} < 1"] = ({i: 0}, EINVAL, body)
    for what, v in (("sigma < 0", {9 + o: -0.1}), ("sigma NaN", {9 + o: np.nan}), ("cfo < 0", {12 + o: -1e-4}),
                    ("cfo inf", {12 + o: np.inf}), ("cfo NaN", {12 + o: np.nan})):
        cases[what] = (v, EINVAL, body)
    return cases


_W, _F = "bad workload arguments", "K >= 0, coh >= 1"
_RW, _RF = "bad workload arguments (1 <= R <= 8)", "bad frame arguments (1 <= R <= 8)"
CASES = {
    "tdec_workload_dev": _symbol_cases(0, _W, "must have 2^bps points)") | {
        "null symbols": ({8: None}, EINVAL, "must have 2^bps points)"),
        "B == 0, null pointers": ({1: 0, 4: None, 8: None, 9: None}, 0, "")},
    "tdec_info_bits_dev": {
        "null handle": ({0: None}, EINVAL, "bad info-bits"), "B < 0": ({1: -1}, EINVAL, "bad info-bits"),
        "cw0 < 0": ({2: -1}, EINVAL, "bad info-bits"), "cw0 < 0, B == 0": ({1: 0, 2: -1}, EINVAL, "bad info-bits"),
        "B == 0, null pointer": ({1: 0, 4: None}, 0, ""), "null bits": ({4: None}, EINVAL, "bad info-bits"),
        "N % 4": ({0: "odd"}, EINVAL, "N % 4 == 0"), "N % 4 comes last": ({0: "odd", 4: None}, EINVAL, "bad info-bits"),
        "N = 1028": ({0: "big"}, EINVAL, "N <= 1024"), "N = 1028 comes last": ({0: "big", 4: None}, EINVAL, "bad info-bits")},
    "tdec_encode_dev": {
        "null handle": ({0: None}, EINVAL, "bad encode"), "B < 0": ({1: -1}, EINVAL, "bad encode"),
        "null handle, B == 0": ({0: None, 1: 0}, EINVAL, "bad encode"),
        "B == 0, null pointers": ({1: 0, 2: None, 3: None}, 0, ""),
        "null bits": ({2: None}, EINVAL, "bad encode"), "null coded": ({3: None}, EINVAL, "bad encode")},
    "tdec_workload_fading_dev": _symbol_cases(0, _W, _F) | _fade_cases(0, _F),
    "tdec_workload_branches_dev": _symbol_cases(1, _RW, _F) | _fade_cases(1, _F) | {
        "R 0": ({2: 0}, EINVAL, _RW), "R 9": ({2: 9}, EINVAL, _RW), "R 9, B == 0": ({1: 0, 2: 9}, EINVAL, _RW)},
    "tdec_workload_frame_dev": _frame_cases(0, "bad frame arguments", "(frame too long)"),
    "tdec_workload_frame_branches_dev": _frame_cases(1, _RF, "(frame or batch too long)") | {
        "R 0": ({4: 0}, EINVAL, _RF), "R 9": ({4: 9}, EINVAL, _RF), "R 9, B == 0": ({3: 0, 4: 9}, EINVAL, _RF),
        "B R > INT32_MAX": ({3: 1 << 30, 4: 4}, EINVAL, "(frame or batch too long)")},
    "tdec_count_errors_dev": {
        "null handle": ({0: None}, EINVAL, "bad count-errors"), "B < 0": ({1: -1}, EINVAL, "bad count-errors"),
        "cw0 < 0": ({2: -1}, EINVAL, "bad count-errors"), "null handle, B == 0": ({0: None, 1: 0}, EINVAL, "bad count-errors"),
        "cw0 < 0, B == 0": ({1: 0, 2: -1}, EINVAL, "bad count-errors"),
        "null bits": ({4: None}, EINVAL, "bad count-errors"), "null counts": ({5: None}, EINVAL, "bad count-errors"),
        "B == 0, null pointers": ({1: 0, 4: None, 5: None}, 0, "")},
}
PARAMS = [(name, case) for name in CASES for case in CASES[name]]


def params(*names):
    """pytest parameters (call, case) of the named calls."""
    return [p for p in PARAMS if p[0] in names]


def check(name, case):
    """Make the call with the case's arguments; assert its return code and message, and that no
    output was written."""
    import torch
    e = _env()
    change, rc, msg = CASES[name][case]
    a = _good(name)
    for i, v in change.items():
        a[i] = e[v].h if isinstance(v, str) else v
    L = N.lib()
    assert getattr(L, name)(*a) == rc, L.tdec_last_error().decode()
    if rc:
        assert msg in L.tdec_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(e["buf"].real).all())
