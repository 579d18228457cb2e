"""Case tables and plain numpy references for the mixer and the carrier loops of the
burst-receive chain (include/modem.h: mdm_mix, mdm_carrier and their _dev forms), beyond what
the golden captures of tests/test_gpu_rx.py reach.  numpy only: no GPU, no torch, no library.
tests/test_rx_loops_host.py checks the tables themselves (the conditions on the designed
inputs, that every wrong variant of the restatement is told from the right one, the census of
detector edges and lane counts); tests/test_gpu_rx_loops.py runs them through the library.

The restatements are written from the contract in include/modem.h, in real arithmetic so that
every rounding is spelled out:
  mixer    out[i] = (sig[i] - dc) * (cos th, sin th), th = w * ((i0 + i) / fs), dc subtracted
           in the signal's precision, the product numpy's complex128 one
  carrier  out[i] = s[i] * exp(-1j*phase) = s[i] * (cos phase, -sin phase);
           freq += (alpha*0.1)*err; phase += alpha*err + freq  (the sum in brackets first);
           err = im*sign(re) | sign(re)*im - sign(im)*re | sin(p - round(p / (pi/4)) * (pi/4)),
           p = arctan2(im, re); np.sign (sign(+-0) = 0, sign(NaN) = NaN), np.round (half to even)
each in float64 and in long double (np.longdouble sin / cos / arctan2 of the same inputs).

Exact cases are compared bit for bit, except that a NaN only has to be a NaN (its sign and
payload are the hardware's).  They need no transcendental function beyond sincos(+-0) = (+-0, 1),
with one family added here: "tiny", one step from |phase0| <= 2^-30, where cos rounds to 1 and
sin to the phase itself (the next terms of both series lie below 2^-60 of the result, less
than 1/256 ulp), so the step is exact with a phase that is not zero.  It is what tells
phase + (alpha*err + freq) from (phase + alpha*err) + freq: from phase0 = 0 the two agree.

TEST INFRASTRUCTURE ONLY."""
import functools
import os
from collections import namedtuple

import numpy as np

C64, C128 = np.complex64, np.complex128
F64, LD = np.float64, np.longdouble
EPS = np.finfo(np.float64).eps
BLOCK, GRID_MAX = 256, 256 * 16                     # modem_kernels.hip: grid_for
STRIDE = GRID_MAX * BLOCK                           # 1 048 576: where k_mix's second trip starts
CR_BLOCK = 64                                       # k_carrier: lanes (streams) per workgroup
CR_BPSK, CR_QUAD, CR_PSK8 = 0, 1, 2
Q = np.pi / 4                                       # 0.7853981633974483, the 8PSK step
ALPHAS = {"sync": 0.03, "BPSK": 0.02, "QPSK": 0.015, "8PSK": 0.01, "16QAM": 0.008, "64QAM": 0.005, "256QAM": 0.003}
ALPHA_KIND = {"sync": CR_BPSK, "BPSK": CR_BPSK, "QPSK": CR_QUAD, "8PSK": CR_PSK8, "16QAM": CR_QUAD, "64QAM": CR_QUAD,
              "256QAM": CR_QUAD}
RTOL, RTOL_N = 1e-10, 2000                          # tests/test_gpu_rx.py: the bound derived there for n <= 2000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rx.npz")


def same_bits(a, b):
    """Equal shape and, read as float64, NaN in the same places and the same bits elsewhere
    (so -0.0 != 0.0; which NaN is not compared)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    fa, fb = a.view(np.float64), b.view(np.float64)
    na, nb = np.isnan(fa), np.isnan(fb)
    return bool(np.array_equal(na, nb) and np.array_equal(fa.view(np.uint64)[~na], fb.view(np.uint64)[~nb]))


def _cplx(re, im):
    out = np.empty(np.shape(re), C128)
    out.real, out.imag = re, im
    return out


# ================================================================ mixer ========================
MixCase = namedtuple("MixCase", "name dtype n i0 w has_dc exact special seed")
MIX_W = (-1j * 2 * np.pi * 5300.0).imag             # what _correct_freq forms for a 5.3 kHz offset
MIX_FS = 200e3
MIX_LENGTHS = (1, 255, 256, 257)
MIX_LARGE = STRIDE + 257                            # blocks 0 and 1 (and one thread of block 2) take a second trip
MIX_I0_BIG, MIX_I0_NEG = 3_000_000_000, -12_345
MIX_VARIANTS = ("dc_in_f64", "i0_int32", "angle_regrouped")
_SPECIAL = (0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -0.75)


@functools.lru_cache(maxsize=None)
def mix_cases():
    out = []

    def add(name, dt, n, i0, w, has_dc, exact, special=False):
        out.append(MixCase(f"{name}-{dt.__name__}-{'dc' if has_dc else 'nodc'}", dt, n, i0, w, has_dc, exact, special,
                           len(out)))
    for dt in (C64, C128):
        for has_dc in (False, True):
            for n in MIX_LENGTHS:
                add(f"w0-n{n}", dt, n, 0, 0.0, has_dc, True)
                add(f"tone-n{n}", dt, n, 1024 * (n % 3), MIX_W, has_dc, False)
            add("w0-special", dt, 300, 0, 0.0, has_dc, True, True)
            add("w0-i0big", dt, 257, MIX_I0_BIG, 0.0, has_dc, True)
            add("w0-i0neg", dt, 257, MIX_I0_NEG, 0.0, has_dc, True)      # th = -0.0: against the restatement only
            add("tone-i0big", dt, 257, MIX_I0_BIG, MIX_W, has_dc, False)
            add("tone-i0neg", dt, 257, MIX_I0_NEG, MIX_W, has_dc, False)
            add("tone-i0negbig", dt, 257, -MIX_I0_BIG, MIX_W, has_dc, False)
        add("w0-large", dt, MIX_LARGE, 0, 0.0, True, True)
        add("tone-large", dt, MIX_LARGE, 0, MIX_W, dt == C128, False)
    return tuple(out)


def mix_inputs(c):
    """(sig, dc): seeded noise around a DC offset; the special case starts with every pair of
    parts from +-0, +-inf, NaN and two finite values.  dc is a complex128 that is no float32."""
    rng = np.random.default_rng([20261101, c.seed])
    sig = (rng.standard_normal(c.n) + 1j * rng.standard_normal(c.n) + (0.3 - 0.2j)).astype(c.dtype)
    if c.special:
        grid = np.array([complex(a, b) for a in _SPECIAL for b in _SPECIAL])
        sig.real[:len(grid)], sig.imag[:len(grid)] = grid.real, grid.imag   # by parts: complex(a, b) keeps every sign
    dc = complex(0.3 + 1e-9 * rng.standard_normal(), -0.2 + 1e-9 * rng.standard_normal()) if c.has_dc else None
    return sig, dc


def mix_centered(sig, dc, variant=None):
    """sig - dc in the signal's precision (numpy's complex subtraction: by parts), as complex128."""
    if dc is None:
        return sig.astype(C128)
    if variant == "dc_in_f64":
        return sig.astype(C128) - C128(dc)
    return (sig - sig.dtype.type(dc)).astype(C128)


def mix_angle(n, i0, w, fs, variant=None):
    idx = np.arange(n, dtype=np.int64) + np.int64(i0)
    if variant == "i0_int32":
        idx = np.arange(n, dtype=np.int64) + np.int64(np.int64(i0).astype(np.int32))
    if variant == "angle_regrouped":
        return (w * idx.astype(F64)) / fs
    return w * (idx.astype(F64) / fs)


def mix_ref(sig, dc, w, fs, i0, T=F64, variant=None):
    """(re, im) of the mixer's output in T: sin / cos in T of the float64 angle, the product in T."""
    d = mix_centered(sig, dc, variant)
    th = mix_angle(len(sig), i0, w, fs, variant).astype(T)
    cs, sn = np.cos(th), np.sin(th)
    re, im = d.real.astype(T), d.imag.astype(T)
    with np.errstate(invalid="ignore"):
        return re * cs - im * sn, re * sn + im * cs


def mix_numpy_w0(sig, dc):
    """numpy's own (sig - dc) * (1 + 0j), the product in complex128 as _correct_freq's is."""
    with np.errstate(invalid="ignore"):
        return mix_centered(sig, dc) * np.full(len(sig), 1 + 0j, C128)


def mix_bound(sig, dc):
    """8 eps |sig - dc| (tests/test_gpu_rx.py: 1 ulp each for the two sin / cos, two roundings of
    the product, doubled), here against the long double restatement."""
    return 8 * EPS * np.abs(mix_centered(sig, dc)).astype(LD)


def mix_distance(y, ref):
    """|y - ref| per sample in long double; ref = (re, im) of mix_ref(..., T=LD)."""
    return np.hypot(y.real.astype(LD) - ref[0], y.imag.astype(LD) - ref[1])


# ================================================================ carrier loops ================
CARRIER_VARIANTS = ("alpha_div_10", "phase_uses_old_freq", "phase_sum_regrouped", "rotate_by_plus_phase", "sign0_is_1",
                    "round_half_away", "quad_terms_swapped", "psk8_step_pi_8")


def _sign(x, variant):
    s = np.sign(x)
    return np.where(x == 0, x.dtype.type(1), s) if variant == "sign0_is_1" else s


def _round(x, variant):
    if variant == "round_half_away":
        return np.sign(x) * np.floor(np.abs(x) + x.dtype.type(0.5))
    return np.round(x)


def carrier_step(sr, si, phase, freq, alpha, kind, T=F64, variant=None):
    """One step of every lane: (re, im) of the output, then the new (phase, freq).  All arrays
    of T, one entry per lane; kind outside 0..2 gives err = NaN (the _dev form's contract)."""
    with np.errstate(all="ignore"):
        cs, sn = np.cos(phase), np.sin(phase)
        msn = sn if variant == "rotate_by_plus_phase" else -sn
        re = sr * cs - si * msn
        im = sr * msn + si * cs
        step = T(Q) / T(2) if variant == "psk8_step_pi_8" else T(Q)
        p = np.arctan2(im, re)
        e2 = np.sin(p - _round(p / step, variant) * step)
        e0 = im * _sign(re, variant)
        if variant == "quad_terms_swapped":
            e1 = _sign(im, variant) * re - _sign(re, variant) * im
        else:
            e1 = _sign(re, variant) * im - _sign(im, variant) * re
        err = np.select([kind == CR_BPSK, kind == CR_QUAD, kind == CR_PSK8], [e0, e1, e2], T(np.nan))
        beta = alpha / T(10) if variant == "alpha_div_10" else alpha * T(0.1)
        new_freq = freq + beta * err
        if variant == "phase_uses_old_freq":
            new_phase = phase + (alpha * err + freq)
        elif variant == "phase_sum_regrouped":
            new_phase = (phase + alpha * err) + new_freq
        else:
            new_phase = phase + (alpha * err + new_freq)
    return re, im, new_phase, new_freq


def carrier_run(syms, ph0, fr0, alpha, kind, T=F64, variant=None):
    """The whole loop over syms [C, n]: (re [C, n], im [C, n], final [C, 2]) in T."""
    syms = np.asarray(syms, C128)
    C, n = syms.shape
    sr, si = syms.real.astype(T), syms.imag.astype(T)
    phase, freq, alpha = (np.array(np.broadcast_to(v, (C,)), T) for v in (ph0, fr0, alpha))
    kind = np.array(np.broadcast_to(kind, (C,)), np.int32)
    re, im = np.empty((C, n), T), np.empty((C, n), T)
    for i in range(n):
        re[:, i], im[:, i], phase, freq = carrier_step(sr[:, i], si[:, i], phase, freq, alpha, kind, T, variant)
    return re, im, np.stack([phase, freq], axis=1)


def carrier_f64(c, variant=None):
    """(out [C, n] complex128, final [C, 2]) of the float64 restatement on a case."""
    re, im, fin = carrier_run(c.syms, c.ph, c.fr, c.al, c.kind, F64, variant)
    return _cplx(re, im), fin


def sides(re, im, kind):
    """What each step's detector decides discontinuously: (sign re, sign im) for BPSK / QUAD (BPSK
    reads the first only), (round(p / (pi/4)), 0) for 8PSK.  Same shapes as re."""
    T = re.dtype.type
    k = np.broadcast_to(np.asarray(kind)[:, None], re.shape)
    with np.errstate(all="ignore"):
        sector = np.round(np.arctan2(im, re) / T(Q))
    a = np.where(k == CR_PSK8, sector, np.sign(re))
    b = np.where(k == CR_QUAD, np.sign(im), 0)
    return a.astype(F64), b.astype(F64)


def margins(re, im, syms, kind):
    """Per step, the distance from the nearest discontinuity of the lane's detector: |re| / |s|
    (BPSK), min(|re|, |im|) / |s| (QUAD), the distance of p / (pi/4) from a half-integer (8PSK)."""
    k = np.broadcast_to(np.asarray(kind)[:, None], re.shape)
    mag = np.abs(syms)
    q = np.arctan2(im, re) / Q
    tie = np.abs((q - np.floor(q)) - 0.5)
    return np.select([k == CR_BPSK, k == CR_QUAD], [np.abs(re) / mag, np.minimum(np.abs(re), np.abs(im)) / mag], tie)


MARGIN = 1e-6


def carrier_distance(y_out, y_fin, ref, syms):
    """Per stream: (max_i |out - ref| / |s[i]|, max over phase, freq of |final - ref| / |ref|), in
    long double; ref = carrier_run(..., T=LD) (or T=F64)."""
    re, im, fin = ref
    d = np.hypot(y_out.real.astype(LD) - re, y_out.imag.astype(LD) - im) / np.abs(syms).astype(LD)
    f = np.abs(y_fin.astype(LD) - fin) / np.abs(fin)
    return np.max(d, axis=1), np.max(f, axis=1)


def carrier_bound(cpu, n):
    """16 times the float64 restatement's own distance from the long double one, floored at the
    rtol of tests/test_gpu_rx.py (derived there for n <= 2000 steps) scaled by n / 2000."""
    return np.maximum(16 * cpu, LD(RTOL * n / RTOL_N))


CarCase = namedtuple("CarCase", "name family exact syms ph fr al kind edge0")
BATCHES = (63, 64, 65, 128, 129, 300)
BATCH_N, LONG_N, LONG_F = 64, 4096, 3.0
NAN_AT = ((17, 5, "re"), (40, 0, "im"), (63, 39, "re"))      # (lane, step, part) of the "nan" case
_CLASSES = ("pos", "neg", "+0", "-0", "+inf", "-inf", "nan")


def _const(kind):
    """The PSK constellation a detector locks on (BPSK, QPSK, 8PSK)."""
    m = (2, 4, 8)[kind]
    return np.exp(1j * (2 * np.pi * np.arange(m) / m + (np.pi / 4 if kind == CR_QUAD else 0.0)))


def _psk_streams(rng, kinds, n, rot, sigma, spin=0.0):
    """Noisy PSK symbols of each lane's own constellation, turned by rot + spin * i."""
    s = np.empty((len(kinds), n), C128)
    for c, k in enumerate(kinds):
        pts = _const(k)
        s[c] = pts[rng.integers(0, len(pts), n)] * np.exp(1j * (rot + spin * np.arange(n)))
    return s + sigma * (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape))


def _class_value(name, rng):
    return {"pos": rng.uniform(0.2, 1.5), "neg": -rng.uniform(0.2, 1.5), "+0": 0.0, "-0": -0.0, "+inf": np.inf,
            "-inf": -np.inf, "nan": np.nan}[name]


def _case(name, family, exact, syms, ph, fr, al, kind, edge0=None):
    C = syms.shape[0]
    ph, fr, al = (np.array(np.broadcast_to(v, (C,)), F64) for v in (ph, fr, al))
    kind = np.array(np.broadcast_to(kind, (C,)), np.int32)
    edge0 = np.zeros(C, bool) if edge0 is None else np.asarray(edge0, bool)
    for a in (syms, ph, fr, al, kind, edge0):
        a.setflags(write=False)
    return CarCase(name, family, exact, syms, ph, fr, al, kind, edge0)


def halfway_symbol():
    """The 8PSK symbol of make_golden_rx.py whose angle / (pi/4) is exactly 0.5 (rx.npz, stream 2)."""
    return complex(np.load(GOLDEN, allow_pickle=False)["crb_in"][2, 0])


def onestep_classes():
    """(kind, class of re, class of im) of the first 98 lanes of the "onestep" case."""
    return [(k, a, b) for k in (CR_BPSK, CR_QUAD) for a in _CLASSES for b in _CLASSES]


def psk8_step_lanes():
    """(sector k, offset d) of the first 45 lanes of the "psk8_step" case."""
    return [(k, f * Q) for k in range(-4, 5) for f in (-0.3, -0.15, 0.0, 0.15, 0.3)]


def _params(rng, C):
    """Random finite alpha and freq0, the latter bounded away from zero."""
    return (rng.uniform(0.003, 0.03, C), rng.choice([-1.0, 1.0], C) * rng.uniform(2e-4, 2e-3, C))


@functools.lru_cache(maxsize=None)
def carrier_cases():
    cases = []
    # ---- exact: one step from phase0 = 0, every class of re and im, then 256 finite lanes
    rng = np.random.default_rng([20261102, 0])
    grid = onestep_classes()
    C = len(grid) + 256
    syms = rng.uniform(0.2, 1.5, C) * np.exp(2j * np.pi * rng.uniform(0, 1, C))
    for c, (_, a, b) in enumerate(grid):
        syms.real[c], syms.imag[c] = _class_value(a, rng), _class_value(b, rng)
    kind = np.array([g[0] for g in grid] + [c % 2 for c in range(256)], np.int32)
    al, fr = _params(rng, C)
    cases.append(_case("onestep", "onestep", True, syms.reshape(C, 1), 0.0, fr, al, kind))
    # ---- exact: one step from a tiny phase (cos = 1, sin = phase)
    rng = np.random.default_rng([20261102, 1])
    C = 256
    syms = rng.uniform(0.2, 1.5, C) * np.exp(2j * np.pi * rng.uniform(0, 1, C))
    ph = rng.choice([-1.0, 1.0], C) * rng.uniform(2.0 ** -31, 2.0 ** -30, C)
    al, fr = _params(rng, C)
    cases.append(_case("tiny", "tiny", True, syms.reshape(C, 1), ph, fr * 1e-6, al, np.arange(C) % 2))
    # ---- exact: alpha = 0 from phase0 = 0, without and with a frequency
    rng = np.random.default_rng([20261102, 2])
    kinds = np.array([0, 1, 2], np.int32)
    syms = _psk_streams(rng, kinds, 300, 0.1, 0.05)
    cases.append(_case("still", "still", True, syms, 0.0, 0.0, 0.0, kinds))
    cases.append(_case("coast", "coast", True, syms, 0.0, np.array([0.01, -0.37, 3.0]), 0.0, kinds))
    # ---- exact between two runs: a NaN sample in one lane of a whole wave
    rng = np.random.default_rng([20261102, 3])
    kinds = (np.arange(CR_BLOCK) % 3).astype(np.int32)
    clean = _psk_streams(rng, kinds, 40, 0.1, 0.02)
    al, fr = _params(rng, CR_BLOCK)
    ph = rng.uniform(-0.15, 0.15, CR_BLOCK)
    dirty = clean.copy()
    for lane, step, part in NAN_AT:
        getattr(dirty, "real" if part == "re" else "imag")[lane, step] = np.nan
    cases.append(_case("nan_clean", "nan", True, clean, ph, fr, al, kinds))
    cases.append(_case("nan", "nan", True, dirty, ph, fr, al, kinds))
    # ---- toleranced: 8PSK, one step from phase0 = 0 around every sector, the branch cut, the tie
    rng = np.random.default_rng([20261102, 4])
    lanes = psk8_step_lanes()
    r = rng.uniform(0.5, 1.5, len(lanes) + 2)
    syms = np.array([r[i] * np.exp(1j * (k * Q + d)) for i, (k, d) in enumerate(lanes)] +
                    [complex(-r[-2], 0.0), complex(-r[-1], -0.0), halfway_symbol()])
    assert np.signbit(syms.imag[-2]) and not np.signbit(syms.imag[-3])
    C = len(syms)
    al, fr = _params(rng, C)
    edge0 = np.zeros(C, bool)
    edge0[-1] = True                                   # the tie is the designed edge
    cases.append(_case("psk8_step", "psk8_step", False, syms.reshape(C, 1), 0.0, fr * 10, al, CR_PSK8, edge0))
    # ---- toleranced: batches around the wave size, kinds cycling lane by lane
    for C in BATCHES:
        rng = np.random.default_rng([20261102, 5, C])
        kinds = (np.arange(C) % 3).astype(np.int32)
        syms = _psk_streams(rng, kinds, BATCH_N, 0.1, 0.02)
        al, fr = _params(rng, C)
        cases.append(_case(f"batch{C}", "batch", False, syms, rng.uniform(-0.15, 0.15, C), fr, al, kinds))
    # ---- toleranced: locked loops at the project's alphas, the symbols spinning 3 rad per symbol
    rng = np.random.default_rng([20261102, 6])
    kinds = np.array([ALPHA_KIND[k] for k in ALPHAS], np.int32)
    syms = _psk_streams(rng, kinds, LONG_N, 0.1, 0.02, spin=LONG_F)
    fr = LONG_F + rng.uniform(-1e-3, 1e-3, len(kinds))
    cases.append(_case("long", "long", False, syms, 0.05, fr, np.array(list(ALPHAS.values())), kinds))
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def carrier_refs(name):
    """Of a toleranced case: the long double run, the float64 run's distance from it per stream
    (out, final) and the bounds that follow.  Shared by the tests; read-only."""
    c = carrier_cases()[name]
    ref = carrier_run(c.syms, c.ph, c.fr, c.al, c.kind, LD)
    out, fin = carrier_f64(c)
    cpu = carrier_distance(out, fin, ref, c.syms)
    n = c.syms.shape[1]
    for a in ref + cpu:
        a.setflags(write=False)
    return ref, cpu, (carrier_bound(cpu[0], n), carrier_bound(cpu[1], n))
