"""Case tables and plain numpy references for the first half of libmodem.so (include/modem.h:
mdm_map, mdm_demod, mdm_fir, mdm_iq_quantize, mdm_iq_dequantize and their _dev forms), aimed at
every dispatch path of mdm_fir_dev and at the edges of the other kernels.  numpy only: no GPU,
no torch.  tests/test_modem_edges_host.py checks the tables themselves (the references against
the C oracle, and that every family tells its operation from a near miss);
tests/test_gpu_modem_edges.py runs them through the library.

  fir_cases / fir_inputs / fir_ref / fir_kernel    integer-valued FIR shapes per kernel family,
                 their inputs, np.convolve of the zero-stuffed input, and the kernel
                 instantiation mdm_fir_dev launches for a shape (its dispatch restated)
  FIR_REAL       real-valued shapes, one per family (tolerance of test_gpu_modem.close, 1e-12)
  map_cases / map_inputs / map_ref                  table[labels]
  demod_cases / demod_ref                           the five hard-decision rules
  quant_cases / quant_ref, dequant_cases / dequant_ref   the IQ sample formats

FIR inputs are integers (x in [-8, 8] + j[-8, 8], taps in [-8, 8]): every product and partial
sum is an exact double, so the kernel, the oracle and numpy agree bit for bit in any summation
order, and an index or phase error cannot hide inside a tolerance.

Two things the IQ quantiser's cases are built around:
  - k_absmax skips |z| for a sample only when the same thread has already seen a larger one,
    and a thread sees a second sample only past 1 048 576 samples (4096 blocks of 256); the
    "long" cases have 2 * 2^20 + 4099 samples, nearly all within the skip margin of the maximum;
  - |Re|, |Im| <= max|sig| < max|sig| + 1e-10, so a scaled part never exceeds 0.95 * 127 =
    120.65: +-127 and the clip cannot be reached through the entry points.  The integer
    boundaries that can be reached (1..120, both signs, both parts) are all in "steps".

TEST INFRASTRUCTURE ONLY."""
import functools
from collections import namedtuple

import numpy as np

C64, C128 = np.complex64, np.complex128
BLOCK, FIR_LDS, TAPS_MAX = 256, 3840, 256          # modem_kernels.hip
GRID_MAX = 256 * 16                                 # blocks of a grid-stride pass (grid_for, k_fir_up, k_fir_dec)
STRIDE = GRID_MAX * BLOCK                           # 1 048 576: where the second trip starts
MAP_SPB, MAP_GRID = 1024, 256 * 8                   # k_map: symbols per block-iteration, blocks


def same_bits(a, b):
    """Equal shape, dtype and bytes (so -0.0 != 0.0 and NaN == NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _uniq(v):
    return list(dict.fromkeys(v))


# ================================================================ FIR ==========================
FirCase = namedtuple("FirCase", "family dtype up down n_x n_taps offset n_out seed")
FIR_FAMILIES = ("up", "dec", "staged", "unstaged", "stride")
FIR_PAST_END = 7 + 7j          # what the "not zeroed" near miss leaves behind the end


def n_valid(c):
    """Outputs of the case that lie inside the full convolution."""
    n_full = (c.n_x - 1) * c.up + c.n_taps
    return max(0, -(-(n_full - c.offset) // c.down))


def _offsets(L, up):
    return [0, (L - 1) // 2, L - 1, L + 3 * up + 1]


def _fir_product(family, ups, downs, n_xs, taps_of):
    """Every (n_x, n_taps) pair of every kernel, twice: the offsets and output counts cycle so
    that each value meets each kernel, each dtype and each tap count."""
    out = []
    for u, (up, down) in enumerate([(a, b) for a in ups for b in downs]):
        for i, n_x in enumerate(n_xs):
            for j, L in enumerate(_uniq(taps_of(up, down))):
                for rep in range(2):
                    off = _offsets(L, up)[(i + 2 * j + u + 2 * rep) % 4]
                    nv = max(0, -(-((n_x - 1) * up + L - off) // down))
                    n_outs = [n for n in (1, nv, nv + 2 * max(up, down) + 1) if n > 0]
                    n_out = n_outs[(i + j + rep) % len(n_outs)]
                    dt = (C64, C128)[(i + j + u + rep) % 2]
                    out.append(FirCase(family, dt, up, down, n_x, L, off, n_out, len(out)))
    return out


def _fir_generic():
    out = []
    for u, (up, down) in enumerate(((3, 2), (5, 3), (2, 3), (3, 1), (7, 1))):
        opb = BLOCK * (4 if down == 1 else 1)
        for i, n_out in enumerate((opb - 1, opb, opb + 1, 3 * opb + 5)):
            for j, L in enumerate((1, 17, 256)):
                off = _offsets(L, up)[(i + j + u) % 4]
                # the input ends two outputs early in half of the cases, 50 samples late in the others
                n_x = max(1, ((n_out - 2) * down + off - L) // up + 1) + (50 if (i + j) % 2 else 0)
                out.append(FirCase("staged", (C64, C128)[(i + j + u) % 2], up, down, n_x, L, off, n_out, 1000 + len(out)))
    return out


def _fir_unstaged():
    out = []
    n_out = 3 * BLOCK + 5
    shapes = [(16, L) for L in (1, 17, 256)] + [(31, L) for L in (1, 17, 256)] + [(15, L) for L in (13, 14, 15)]
    for u, (down, L) in enumerate(shapes):
        for k, dt in enumerate((C64, C128)):
            off = _offsets(L, 1)[(u + k) % 4]
            n_x = max(1, (n_out - 2) * down + off - L + 1) + (50 if (u + k) % 2 else 0)
            out.append(FirCase("unstaged", dt, 1, down, n_x, L, off, n_out, 2000 + len(out)))
    return out


@functools.lru_cache(maxsize=None)
def fir_cases(family):
    if family == "up":
        return tuple(_fir_product("up", (2, 4, 8, 16), (1,), (1, 2, 255, 256, 257, 600),
                                  lambda up, down: (1, up - 1, up, up + 1, 101, 256)))
    if family == "dec":
        return tuple(_fir_product("dec", (1,), (1, 2, 4, 8), (1, 255, 256, 257, 513, 2000),
                                  lambda up, down: (1, 2, down, 255, 256)))
    if family == "staged":
        return tuple(_fir_generic())
    if family == "unstaged":     # with the staging threshold: down 15, 13 and 14 taps are still staged
        return tuple(_fir_unstaged())
    assert family == "stride"
    n_x = STRIDE + 300
    return (FirCase("stride", C64, 2, 1, n_x, 5, 2, (n_x - 1) * 2 + 5 - 2, 3000),          # n_x + 1 periods
            FirCase("stride", C64, 1, 1, STRIDE + 777, 5, 2, STRIDE + 777 + 5 - 1 - 2 + 3, 3001))


# real-valued inputs (standard normal), one per kernel family: fma against the oracle's mul + add
FIR_REAL = (FirCase("up", C64, 4, 1, 3001, 101, 50, 3001 * 4, 4000), FirCase("up", C128, 2, 1, 2999, 33, 0, 6030, 4001),
            FirCase("dec", C128, 1, 2, 4001, 49, 48, 2001, 4002), FirCase("dec", C64, 1, 1, 3000, 101, 50, 3000, 4003),
            FirCase("staged", C64, 3, 2, 2001, 17, 8, 3010, 4004), FirCase("staged", C128, 7, 1, 500, 65, 0, 3558, 4005),
            FirCase("unstaged", C128, 1, 16, 16000, 49, 24, 1003, 4006))


def fir_inputs(c, real=False):
    """(x, taps) of a case: integers, or standard normal values for the FIR_REAL cases."""
    rng = np.random.default_rng(1000003 + c.seed)
    if real:
        x = rng.standard_normal(c.n_x) + 1j * rng.standard_normal(c.n_x)
        return x.astype(c.dtype), rng.standard_normal(c.n_taps)
    x = rng.integers(-8, 9, c.n_x) + 1j * rng.integers(-8, 9, c.n_x)
    h = rng.integers(-8, 9, c.n_taps).astype(np.float64)
    h[h == 0] = 3.0           # no tap drops out by chance
    return x.astype(c.dtype), h


def fir_ref(x, h, up, down, offset, n_out, variant=None):
    """Zero-stuff x by up, np.convolve with h in float64, [offset::down][:n_out], zero-extended.
    variant: a near miss (test_modem_edges_host.py): "offset+1", "phase" (the first tap of every
    output one too far), "drop_last_tap", "past_end" (the outputs behind the end left alone)."""
    x = np.asarray(x).astype(C128)
    h = np.array(h, np.float64)
    if variant == "drop_last_tap":
        h[-1] = 0.0
    if variant == "offset+1":
        offset += 1
    shift = 1 if variant == "phase" else 0
    xu = np.zeros((len(x) - 1) * up + 1 + shift, C128)
    xu[shift::up] = x
    full = np.empty(len(xu) + len(h) - 1, C128)
    full.real = np.convolve(xu.real, h)
    full.imag = np.convolve(xu.imag, h)
    y = full[offset::down][:n_out]
    out = np.full(n_out, FIR_PAST_END if variant == "past_end" else 0, C128)
    out[:len(y)] = y
    return out + 0.0          # -0.0 + 0.0 = +0.0: the kernels and the oracle start their sums at +0.0


def fir_case_ref(c, variant=None):
    x, h = fir_inputs(c)
    return fir_ref(x, h, c.up, c.down, c.offset, c.n_out, variant)


def fir_kernel(c):
    """The instantiation mdm_fir_dev launches for the shape (modem_api.hip, in its order)."""
    t = "float" if c.dtype == C64 else "double"
    if c.down == 1 and c.up in (2, 4, 8, 16):
        return f"k_fir_up<{t},{c.up}>"
    if c.up == 1 and c.down in (1, 2, 4, 8):
        return f"k_fir_dec<{t},{c.down}>"
    opb = BLOCK * (4 if c.down == 1 else 1)
    span = ((opb - 1) * c.down + c.n_taps - 1) // c.up + 2
    return f"k_fir<{t},{'true' if span <= FIR_LDS else 'false'}>"


def fir_second_trip(c):
    """Does a block of the case's kernel run its grid-stride loop a second time?"""
    k = fir_kernel(c)
    if k.startswith("k_fir_up"):
        return (c.n_out - 1 + c.offset) // c.up + 1 > STRIDE
    return k.startswith("k_fir_dec") and c.n_out > STRIDE


# ================================================================ mapper =======================
MapCase = namedtuple("MapCase", "bps dtype n_bits seed")
MAP_OFFSETS = (0, 1, 8, 15, 16)                     # byte offsets of the device bits (map_device)
MAP_LARGE = (MapCase(1, C64, MAP_GRID * MAP_SPB + 1500, 77), MapCase(8, C64, 8 * (MAP_GRID * MAP_SPB + 1500), 78))


@functools.lru_cache(maxsize=None)
def map_cases():
    out = []
    for dt, top in ((C64, 8), (C128, 7)):
        for bps in range(1, top + 1):
            spb = MAP_SPB * bps
            for n in _uniq((1, bps - 1, bps, spb - 1, spb, spb + 1, 3 * spb + bps // 2 + 1)):
                if n > 0:
                    out.append(MapCase(bps, dt, n, len(out)))
    return tuple(out)


def map_inputs(c):
    """(bits, table): random bits and 2^bps random points (distinct: the host test checks)."""
    rng = np.random.default_rng(2000003 + 131 * c.seed + c.bps)
    M = 1 << c.bps
    table = (rng.standard_normal(M) + 1j * rng.standard_normal(M)).astype(c.dtype)
    return rng.integers(0, 2, c.n_bits).astype(np.uint8), table


def map_ref(bits, bps, table, variant=None):
    """table[labels]: labels MSB first, the last one zero padded.  variant: "lsb_first", "pad_ones"."""
    bits = np.asarray(bits, np.int64)
    pad = np.full((-len(bits)) % bps, 1 if variant == "pad_ones" else 0, np.int64)
    w = 1 << (np.arange(bps) if variant == "lsb_first" else np.arange(bps - 1, -1, -1))
    return np.asarray(table)[np.concatenate([bits, pad]).reshape(-1, bps) @ w]


# ================================================================ hard demodulators ============
GT0, QPSK, PSK8, QAM_AXIS, ARGMIN = 0, 1, 2, 3, 4
DemodCase = namedtuple("DemodCase", "family name kind bps syms labels scale cons nan_raises")
DEMOD_FAMILIES = ("signs", "psk8_exact", "psk8_special", "psk8_boundary", "qam_axis", "argmin")
QAM_SCALE = {2: np.sqrt(2.0), 4: np.sqrt(10.0), 6: np.sqrt(42.0), 8: np.sqrt(170.0)}
GRAY = {1: [1, 0], 2: [0, 1, 3, 2], 3: [0, 1, 3, 2, 6, 7, 5, 4],
        4: [0, 1, 3, 2, 6, 7, 5, 4, 12, 13, 15, 14, 10, 11, 9, 8]}
INV_GRAY = {k: [g.index(i) for i in range(len(g))] for k, g in GRAY.items()}
NAN, INF = np.nan, np.inf


def _real(dt):
    return np.float32 if dt == C64 else np.float64


def _cplx(re, im, dt):
    z = np.empty(len(re), dt)
    z.real, z.imag = re, im
    return z


def _grid(vals, dt):
    """Every (re, im) pair of the values."""
    v = np.asarray(vals, _real(dt))
    return _cplx(np.repeat(v, len(v)), np.tile(v, len(v)), dt)


def steps(x, n, T):
    """x in T and its n neighbours on either side (np.nextafter)."""
    x = T(x)
    lo, hi = [x], [x]
    for _ in range(n):
        lo.append(np.nextafter(lo[-1], T(-INF)))
        hi.append(np.nextafter(hi[-1], T(INF)))
    return np.array(lo[:0:-1] + hi, T)


def qam_axis_values(bps, scale, dt):
    """Axis values whose (x * scale + L - 1) / 2 lies at every integer and every half-integer
    from -1 to L (and three floats either side of each, so the exact point is there wherever
    one exists), then what clips and what does not convert."""
    T, L = _real(dt), 1 << (bps // 2)
    vals = [steps((2.0 * t - (L - 1)) / scale, 3, T) for t in np.arange(-1.0, L + 0.25, 0.5)]
    big = 3e38 if dt == C64 else 1e300
    return np.concatenate(vals + [np.array([INF, -INF, big, -big], T)])


def qam_axis_position(x, bps, scale):
    """(x * scale + L - 1) / 2 as the reference forms it (float64)."""
    return (np.asarray(x).astype(np.float64) * scale + ((1 << (bps // 2)) - 1)) / 2


def argmin_cons(bps):
    """2^bps points on the odd integers (a 2^ceil x 2^floor grid): midpoints are exact ties."""
    a, b = (bps + 1) // 2, bps // 2
    xs, ys = np.arange(-(1 << a) + 1, 1 << a, 2.0), np.arange(-(1 << b) + 1, 1 << b, 2.0)
    return (np.repeat(xs, len(ys)) + 1j * np.tile(ys, len(xs))).astype(C128)


def _psk8_points(fracs, radii, dt):
    k = np.arange(8)[:, None, None]
    ang = (k + np.asarray(fracs)[None, :, None]) * (np.pi / 4)
    z = np.asarray(radii)[None, None, :] * np.exp(1j * ang)
    return z.ravel().astype(dt)


@functools.lru_cache(maxsize=None)
def demod_cases(family):
    out = []

    def add(name, kind, bps, syms, labels=None, scale=0.0, cons=None, nan_raises=1):
        out.append(DemodCase(family, name, kind, bps, syms, labels, scale, cons, nan_raises))

    for dt in (C64, C128):
        tag = "c64" if dt == C64 else "c128"
        den = 1e-45 if dt == C64 else 5e-324
        if family == "signs":
            g = _grid([0.0, -0.0, den, -den, INF, -INF, NAN, 1.0, -1.0], dt)
            add(f"gt0 {tag}", GT0, 1, g)
            add(f"qpsk {tag}", QPSK, 2, g)
        elif family == "psk8_exact":      # the centres and up to 0.49 of a sector either side
            add(f"{tag}", PSK8, 3, _psk8_points([-0.49, -0.25, 0.0, 0.25, 0.49], [0.5, 1.0, 3.0], dt), INV_GRAY[3])
            add(f"{tag} identity", PSK8, 3, _psk8_points([-0.49, 0.0, 0.49], [1.0], dt), None, nan_raises=0)
        elif family == "psk8_special":    # the axes with signed zeros, the origin, infinities, NaN
            g = _grid([0.0, -0.0, 1.0, -1.0, INF, -INF, den, -den], dt)
            n = _grid([NAN, 0.0, 1.0, -INF], dt)
            for raises in (0, 1):
                add(f"{tag} finite, raises {raises}", PSK8, 3, g, INV_GRAY[3], nan_raises=raises)
                add(f"{tag} NaN, raises {raises}", PSK8, 3, n, INV_GRAY[3], nan_raises=raises)
        elif family == "psk8_boundary":   # on, 1e-6 and 1e-3 of a sector off the boundaries
            f = [0.5 + d for d in (0.0, 1e-6, -1e-6, 1e-3, -1e-3)]
            add(f"{tag}", PSK8, 3, _psk8_points(f, [0.7, 1.0, 2.5], dt), INV_GRAY[3])
        elif family == "qam_axis":
            for bps in (2, 4, 6, 8):
                for scale in (QAM_SCALE[bps], 2.0):      # with scale 2 every tie is exact in both dtypes
                    v = qam_axis_values(bps, scale, dt)
                    add(f"{tag} bps {bps} scale {scale:.3f}", QAM_AXIS, bps, _cplx(v, v[::-1], dt),
                        INV_GRAY[bps // 2], scale)
                n = _grid([NAN, 0.3, -0.3], dt)           # NaN in one axis only, and in both
                add(f"{tag} bps {bps} NaN", QAM_AXIS, bps, n, INV_GRAY[bps // 2], QAM_SCALE[bps])
        else:
            assert family == "argmin"
            rng = np.random.default_rng(5 + (dt == C128))
            for bps in range(1, 7):
                c = argmin_cons(bps)
                lim = float(np.max(c.real)) + 1.5
                rnd = (rng.uniform(-lim, lim, 4000) + 1j * rng.uniform(-lim, lim, 4000)).astype(dt)
                add(f"{tag} bps {bps} random", ARGMIN, bps, rnd, cons=c)
                e = np.arange(-(1 << ((bps + 1) // 2)) - 2, (1 << ((bps + 1) // 2)) + 3, 1.0)
                add(f"{tag} bps {bps} ties", ARGMIN, bps, _grid(e, dt), cons=c)      # even coordinates: 2 or 4 nearest
                add(f"{tag} bps {bps} non-finite", ARGMIN, bps, _grid([INF, -INF, NAN, 0.5], dt), cons=c)
    return tuple(out)


def _label_bits(lab, n):
    return ((np.asarray(lab, np.int64)[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(np.uint8)


def demod_ref(c, variant=None):
    """(bits uint8 [n * bps], NaN count) of a case in plain numpy.  variant: "half_away" and
    "no_clip" (QAM_AXIS), "last_min" (ARGMIN)."""
    s = np.asarray(c.syms)
    n = len(s)
    with np.errstate(all="ignore"):
        if c.kind == GT0:
            return (s.real > 0).astype(np.uint8), 0
        if c.kind == QPSK:
            return np.stack([s.real < 0, s.imag < 0], 1).astype(np.uint8).ravel(), 0
        if c.kind == PSK8:
            T = _real(s.dtype.type)
            ph = np.angle(s).astype(T)
            ph = np.where(ph < 0, ph + T(2 * np.pi), ph)
            r = np.round(ph / T(np.pi / 4))
            nan = np.isnan(r)
            idx = np.where(nan, 0, r).astype(np.int64) % 8
            lab = np.arange(8) if c.labels is None else np.asarray(c.labels)
            return _label_bits(lab[idx], 3).ravel(), int(nan.sum()) * c.nan_raises
        if c.kind == QAM_AXIS:
            K = c.bps // 2
            L = 1 << K
            v = (np.stack([s.real, s.imag], 1).astype(np.float64) * c.scale + (L - 1)) / 2
            q = np.trunc(v + np.copysign(0.5, v)) if variant == "half_away" else np.round(v)
            nan = np.isnan(q)
            q = np.where(nan, 0.0, q)
            if variant == "no_clip":
                idx = np.where(np.isfinite(q), np.mod(q, L), np.clip(q, 0, L - 1)).astype(np.int64)
            else:
                idx = np.clip(q, 0, L - 1).astype(np.int64)
            return _label_bits(np.asarray(c.labels)[idx].ravel(), K).reshape(n, 2 * K).ravel(), int(nan.sum())
        d = np.abs(s.astype(C128)[:, None] - c.cons[None, :])
        idx = d.shape[1] - 1 - np.argmin(d[:, ::-1], 1) if variant == "last_min" else np.argmin(d, 1)
        return _label_bits(idx, c.bps).ravel(), 0


DEMOD_ALIGN = tuple((bps, off) for bps in (2, 4, 8) for off in range(4))     # out slices of demod_device
DEMOD_LARGE = STRIDE + 777


def demod_large(which):
    """1 048 576 + 777 noisy symbols of a 1-bit rule ("gt0") and of 256QAM ("qam256"), complex64."""
    rng = np.random.default_rng(41)
    z = (rng.uniform(-1.3, 1.3, DEMOD_LARGE) + 1j * rng.uniform(-1.3, 1.3, DEMOD_LARGE)).astype(C64)
    if which == "gt0":
        return DemodCase("large", "gt0", GT0, 1, z, None, 0.0, None, 1)
    return DemodCase("large", "qam256", QAM_AXIS, 8, z, INV_GRAY[4], QAM_SCALE[8], None, 1)


# ================================================================ IQ formats ===================
QUANT_MARGIN = {C64: 1e-5, C128: 1e-9}              # k_absmax
QUANT_LONG = 2 * STRIDE + 4099
QUANT_NAMES = ("n1", "zeros", "gauss", "circle", "near_circle", "steps", "nan", "posinf", "neginf", "denormal",
               "long")


def _quant_scaled(x, d, T):
    """A real or imaginary part as the quantiser scales it before the clip: numpy's complex
    division by (d + 0j) is a product with 1 / d, then * 0.95, then * 127, all in T."""
    return np.asarray(x, T) * (T(1) / T(d)) * T(0.95) * T(127)


def _quant_steps(d, T):
    """Parts that land on, just below and just above every integer 1..120 after scaling by a
    maximum of d - 1e-10, with both signs."""
    v = np.concatenate([steps(T(k) / T(127) / T(0.95) * T(d), 6, T) for k in range(1, 121)])
    return np.concatenate([v, -v])


def _near_circle(n, dt, rng, spread):
    T = _real(dt)
    th = rng.uniform(0, 2 * np.pi, n)
    r = 1.0 - spread * rng.uniform(0, 1, n)
    return _cplx((r * np.cos(th)).astype(T), (r * np.sin(th)).astype(T), dt)


@functools.lru_cache(maxsize=None)
def quant_cases(dt):
    """{name: signal} of one dtype."""
    T, m = _real(dt), QUANT_MARGIN[dt]
    rng = np.random.default_rng(17 + (dt == C128))
    eps = np.finfo(T).eps
    out = {"n1": np.array([0.3 - 0.7j], dt), "zeros": np.zeros(1000, dt),
           "gauss": (rng.standard_normal(3001) + 1j * rng.standard_normal(3001)).astype(dt)}
    th = 2 * np.pi * np.arange(5000) / 5000
    k = (1 + (np.arange(5000) % 4) * eps).astype(T)      # moduli 0, 1, 2, 3 ulp apart, and what rounding adds
    out["circle"] = _cplx(np.cos(th).astype(T) * k, np.sin(th).astype(T) * k, dt)
    out["near_circle"] = _near_circle(5000, dt, rng, 2 * m)
    one = np.array([1.0], T)
    st = _quant_steps(T(1) + T(1e-10), T)
    z = np.zeros(len(st), T)
    out["steps"] = np.concatenate([_cplx(one, 0 * one, dt), _cplx(st, z, dt), _cplx(z, st, dt), _cplx(st, st[::-1] / 2, dt)])
    g = out["gauss"][:257]
    for name, v in (("nan", NAN), ("posinf", INF), ("neginf", -INF)):
        s = g.copy()
        s[100] = complex(v, 0.25) if name != "neginf" else complex(0.25, v)
        out[name] = s
    if dt == C64:
        out["denormal"] = _cplx(np.array([1e-45, -3e-42, 1e-39, 0.0, 7e-41], T), np.array([0.0, 2e-45, -1e-39, 5e-40, 0], T), dt)
    # past 2 * 2^20 samples every thread of k_absmax sees three: nearly all within the margin of the
    # maximum (nothing may be skipped), a quarter at half the modulus (skipped wherever they come
    # second), the largest sample (4 ulp above the rest, the second one of its thread) and the
    # integer boundaries under that maximum
    peak = T(1) + 4 * eps
    st = _quant_steps(peak + T(1e-10), T)
    big = _near_circle(QUANT_LONG, dt, rng, 2 * m)
    big[::4] *= T(0.5)
    big[:len(st)] = _cplx(st, z, dt)
    big[len(st):2 * len(st)] = _cplx(z, st, dt)
    big[STRIDE + 12345] = peak
    out["long"] = big
    return out


def quant_ref(sig, variant=None):
    """sig / (max|sig| + 1e-10) * 0.95 in the signal's precision, * 127, clip, truncate; int8
    interleaved.  variant: "round" (to nearest instead of truncation), "skip_max" (the maximum
    misses one sample of the largest modulus)."""
    sig = np.asarray(sig)
    T = _real(sig.dtype.type)
    with np.errstate(all="ignore"):
        a = np.abs(sig)
        if variant == "skip_max" and len(a) > 1:
            a = np.delete(a, np.argmax(np.where(np.isnan(a), INF, a)))
        d = T(np.max(a)) + T(1e-10)
        rat = T(0) / d                                   # numpy's complex division by (d + 0j), Smith's method
        scl = T(1) / (d + T(0) * rat)
        qr, qi = (sig.real + sig.imag * rat) * scl, (sig.imag - sig.real * rat) * scl
        pr, pi = qr * T(0.95) - qi * T(0), qr * T(0) + qi * T(0.95)
        out = np.empty(2 * len(sig), np.int8)
        for k, p in enumerate((pr, pi)):
            v = np.clip(np.where(np.isnan(p), T(0), p * T(127)), -127, 127)      # astype(int8) of NaN is 0 on x86
            out[k::2] = (np.rint(v) if variant == "round" else np.trunc(v)).astype(np.int8)
    return out


DEQUANT_PAIRS = (1, 7, 8, 9, 8 * 256 + 3)
DEQUANT_OFFSETS = ((0, 0), (2, 0), (0, 1), (6, 1), (16, 2))      # (raw bytes, out samples): only the first and last keep 16 B


@functools.lru_cache(maxsize=None)
def dequant_cases():
    """{name: raw bytes}: every byte pair, then the short counts around the 8-sample vector step."""
    a = np.arange(65536)
    allp = np.stack([a >> 8, a & 255], 1).astype(np.uint8).ravel()
    rng = np.random.default_rng(23)
    out = {"all pairs": allp}
    for n in DEQUANT_PAIRS:
        out[f"{n} pairs"] = rng.integers(0, 256, 2 * n).astype(np.uint8)
    return out


def dequant_ref(raw, mid=127.5):
    """(raw.astype(float32) - 127.5) / 127.5, I from the even bytes and Q from the odd ones."""
    raw = np.asarray(raw, np.uint8)
    m = np.float32(mid)
    return _cplx((raw[0::2].astype(np.float32) - m) / m, (raw[1::2].astype(np.float32) - m) / m, C64)
