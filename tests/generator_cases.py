"""Designed cases of the counter-based workload generator (modulations_amd/csrc/tdec_workload.hip:
info bits, encoder, mapper, AWGN, fading gains, receive branches, pilot framing, k_count_errors)
with their numpy references, for tests/test_generator_cases_host.py (which proves that the tables
do what they claim and that each family rejects the wrong variants listed for it) and
tests/test_gpu_generator.py (which runs them through the C ABI and workload.py).

TEST INFRASTRUCTURE.  The references are oracle/workload_ref.py, tests/fading_ref.py and
tests/pilot_csi_ref.py: Philox words, the device's float32 uniform, everything behind it in float64.
Beside them stands a second restatement that steps every operation in float32 (box_muller32, sin and
cos of pi * 2 u2 evaluated in float64 and rounded once).  It has two uses: its distance to the
float64 reference, in units of the Box-Muller radius, is the measured `tau` of the tolerance, and
with a `variant` it plays a device that is wrong in one named way.

Tolerance of a noisy sample, per component:  |device - ref64| <= ulp32(y_ref) / 2 + 4 tau rad_ref.
The half ulp is the final float32 addition (table point or h x, plus noise); `rad_ref` is the
reference's radius, not the component, which can be near zero; 4 tau allows the device's logf, sqrtf
and sincospif a couple of ulp each where the float32 numpy steps are within one.  tau is never taken
from a device.
"""
import functools

import numpy as np

import fading_ref as F
import pilot_csi_ref as P
from oracle import workload_ref as W

F32, F64 = np.float32, np.float64
_M = np.uint64(0xFFFFFFFF)
NOISE, FADE, PILOT = W.NOISE_DOMAIN, F.FADE_DOMAIN, P.PILOT_DOMAIN
TOP = 2 ** 24 - 1                                  # x >> 8 of the draw whose uniform is exactly 1

# ---- counter family -------------------------------------------------------------------------------
B = 130                                            # two full tiles and a partial one
CW0S = (0, 2 ** 32 - 40, 2 ** 40 + 12345, 2 ** 63 - 200)   # the second: the carry into counter word 1 inside a tile
SEEDS = (4242, 0xDEADBEEF12345, 2 ** 64 - 1)
COUNTERS = [(cw0, seed) for cw0 in CW0S for seed in SEEDS]
COUNTER_IDS = [f"cw0={cw0:#x}-seed={seed:#x}" for cw0, seed in COUNTERS]
BULK = dict(n=48, rate="1/3", mod="16QAM", S=72, ebn0=2.0, K=4.0, coh=5, R=3)   # the streams' shape
FRAME = dict(plen=3, dlen=16, ebn0=6.0, cfo=1e-3)   # S = 72: 4 segments of 16 and one of 8; 18 pilots, blocks at odd k
VARIANCE = dict(n=48, rate="1/3", ebn0=3.0, seed=0xDEADBEEF12345, cw0=2 ** 40 + 12345)

# ---- tail family ------------------------------------------------------------------------------------
# (domain, codeword - TAIL_CW0, element s of pair 0, which uniform, its x >> 8), found once by a search of
# the codewords from TAIL_CW0 on over counter word 2 = 0; the host test recomputes every row.
TAIL_SEED, TAIL_CW0, TAIL_LANE = 0xC0FFEE1234567, 2 ** 40, 37
TAILS = [
    ("noise", 160280, 1, "u2", 16777212), ("noise", 2041687, 0, "u2", 3), ("noise", 3497369, 1, "u2", 1),
    ("noise", 3553443, 0, "u1", 1), ("noise", 4334317, 0, "u2", 0), ("noise", 5212642, 0, "u1", 16777212),
    ("noise", 5374029, 1, "u1", 16777215), ("noise", 6428308, 1, "u1", 16777215), ("noise", 6503915, 1, "u2", 16777213),
    ("noise", 7940872, 1, "u2", 16777214), ("noise", 8575726, 0, "u1", 3), ("noise", 8809032, 1, "u1", 16777214),
    ("noise", 38621309, 0, "u2", 16777215),
    ("gain", 717123, 0, "u2", 16777215), ("gain", 1183262, 0, "u2", 16777214), ("gain", 2347433, 0, "u1", 1),
    ("gain", 2546064, 0, "u1", 16777212), ("gain", 3165468, 0, "u2", 0), ("gain", 3292792, 1, "u1", 0),
    ("gain", 3716044, 1, "u2", 1), ("gain", 4118745, 1, "u1", 16777213), ("gain", 4509908, 0, "u1", 3),
    ("gain", 4696802, 0, "u2", 16777215), ("gain", 34027283, 1, "u1", 16777215),
]
TAIL_IDS = [f"{d}-{c}-{s}-{r}-{v}" for d, c, s, r, v in TAILS]
TAIL_K = 4.0                                       # the gain rows' Rician factor (los 0.894: a top u1 is visibly `los`)

# ---- mapper family ------------------------------------------------------------------------------------
MAPPER_B = 70
MAPPER = [(1024, "1/3", 1), (4, "3/4", 2), (52, "1/3", 5), (140, "3/4", 3), (4, "1/3", 4), (64, "1/2", 6),
          (100, "2/3", 7), (212, "3/4", 8), (1024, "3/4", 7), (48, "1/3", 8), (36, "1/2", 5), (8, "2/3", 1)]
MAPPER_IDS = [f"N={n}-r={r}-bps={b}" for n, r, b in MAPPER]

# ---- fading family ------------------------------------------------------------------------------------
FADING = dict(n=212, rate="3/4", mod="8PSK", S=195, B=70, ebn0=4.0, seed=0xDEADBEEF12345, cw0=2 ** 32 - 40)
_S = FADING["S"]                                   # odd: the last symbol uses words x, y of a pair on its own
FADING_ONE = [(K, coh) for K in (0.0, 4.0, 1e30) for coh in (1, 63, 65, _S, _S + 1)]
FADING_BRANCHES = [(4.0, 63, 1), (4.0, 65, 1), (4.0, 63, 3), (4.0, 65, 3), (4.0, 63, 8), (4.0, 65, 8), (0.0, 1, 3),
                   (1e30, _S + 1, 8), (0.0, _S, 3)]

# ---- error-count family -------------------------------------------------------------------------------
COUNT_N = (4, 50, 128, 130, 213, 1024)             # 128: one 256-bit sweep; 130: one lane more; 213: 2N % 4 != 0
# The family runs at the largest cw0, 2^63 - 200, and cw0 + rows of a call must stay below 2^63 (cw0 is an int64
# in the ABI): its 2N rows go in calls of at most 190 rows, all at that cw0, in place of one call at a lower cw0.
# k_count_errors is one block per row, so no path depends on the rows of a call; the counter family runs it at
# every (cw0, seed) besides.
COUNT_CW0, COUNT_SEED, COUNT_CHUNK = CW0S[-1], SEEDS[1], 190


def cws(cw0, n):
    """uint64 [n]: the global codeword indices cw0 .. cw0 + n - 1."""
    return np.uint64(cw0) + np.arange(n, dtype=np.uint64)


def made_up_perm(n):
    """Values in [0, N), no permutation in general (the handle takes any; the reference's own tables
    repeat values too)."""
    i = np.arange(n, dtype=np.int64)
    return ((7 * i * i + 3 * i + 1) % n).astype(np.int32)


# ---- the streams' words, with the counter variants ----------------------------------------------------
def words(cw_global, n, seed, domain, variant=None):
    """oracle.workload_ref.stream_words, or wrong in one way: "ctr1" counter word 1 dropped, "key1" key
    word 1 dropped, "s" element s in place of s >> 1 in counter word 2, "swap" words x, y and z, w
    exchanged between even and odd elements."""
    cw = np.asarray(cw_global, np.uint64)[:, None]
    s = np.arange(n, dtype=np.uint64)[None, :]
    hi = np.zeros_like(cw) if variant == "ctr1" else cw >> np.uint64(32)
    k1 = 0 if variant == "key1" else seed >> 32
    c2 = s if variant == "s" else s >> np.uint64(1)
    r = W.philox4x32_10(cw & _M, hi, c2, domain, seed & 0xFFFFFFFF, k1)
    odd = np.broadcast_to((s & np.uint64(1)).astype(bool), r[0].shape)
    if variant == "swap":
        odd = ~odd
    return np.where(odd, r[2], r[0]), np.where(odd, r[3], r[1])


def info_bits(cw_global, n_couples, seed, variant=None):
    """oracle.workload_ref.info_bits, or with counter word 1 ("ctr1") or key word 1 ("key1") dropped."""
    cw = np.asarray(cw_global, np.uint64)
    if variant == "ctr1":
        cw = cw & _M
    return W.info_bits(cw, n_couples, seed & 0xFFFFFFFF if variant == "key1" else seed)


# ---- Box-Muller: the float64 reference and the float32 restatement ------------------------------------
def radius(a, sigma):
    """The float64 reference's radius float32(sigma) sqrt(-2 ln u1)."""
    return F64(F32(sigma)) * np.sqrt(-2.0 * np.log(W.uniform24(a)) + 0.0)


def box_muller32(a, b, sigma, variant=None):
    """(re, im) float32: the kernel's expression with every operation stepped in float32; sin and cos of
    pi * (2 u2) in float64, rounded once.  Variants: "sincos" sine and cosine exchanged, "nohalf" u without
    the + 0.5, "u64" u formed in float64 (and, to keep it there, everything behind it: the earlier
    restatement, rounded to float32 at the end)."""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    if variant == "u64":
        u1, u2 = ((a >> 8).astype(F64) + 0.5) * 2.0 ** -24, ((b >> 8).astype(F64) + 0.5) * 2.0 ** -24
        rad = F64(F32(sigma)) * np.sqrt(-2.0 * np.log(u1))
        return (rad * np.cos(2 * np.pi * u2)).astype(F32), (rad * np.sin(2 * np.pi * u2)).astype(F32)
    half = F32(0.0 if variant == "nohalf" else 0.5)
    u1 = ((a >> 8).astype(F32) + half) * F32(2.0 ** -24)
    u2 = ((b >> 8).astype(F32) + half) * F32(2.0 ** -24)
    with np.errstate(divide="ignore"):
        rad = F32(sigma) * np.sqrt(F32(-2.0) * np.log(u1))
    assert rad.dtype == F32
    sn, cs = W.sincospi((F32(2.0) * u2).astype(F64))
    sn, cs = sn.astype(F32), cs.astype(F32)
    if variant == "sincos":
        sn, cs = cs, sn
    return rad * cs, rad * sn


def noise(cw_global, n, seed, sigma, domain=NOISE, branch=0):
    """(noise complex128 [len(cw), n], radius float64): the float64 reference of a noise stream."""
    a, b = W.stream_words(cw_global, n, seed, domain | (branch << 16))
    return W.box_muller(a, b, sigma), radius(a, sigma)


def noise32(cw_global, n, seed, sigma, domain=NOISE, branch=0, variant=None):
    """The float32 restatement of the same, (re, im) float32; `variant` as in words and box_muller32."""
    wv = variant if variant in ("ctr1", "key1", "s", "swap") else None
    a, b = words(cw_global, n, seed, domain | (branch << 16), wv)
    return box_muller32(a, b, sigma, None if wv else variant)


SQRT_HALF = F32(0.70710678118654752)


def gains(cw_global, n_blocks, seed, K, branch=0):
    """(gains complex128, radius scat * rad float64): tests/fading_ref.gains and the tolerance's radius."""
    a, _ = W.stream_words(cw_global, n_blocks, seed, FADE | (branch << 16))
    return F.gains(cw_global, n_blocks, seed, K, branch), F.los_scat(K)[1] * radius(a, SQRT_HALF)


def gains32(cw_global, n_blocks, seed, K, branch=0, variant=None):
    """complex64: the kernel's los + scat * (rad * cs), scat * (rad * sn) stepped in float32."""
    re, im = noise32(cw_global, n_blocks, seed, SQRT_HALF, FADE, branch, variant)
    los, scat = (F32(v) for v in F.los_scat(K))
    return to_c64(los + scat * re, scat * im)


def to_c64(re, im):
    out = np.empty(np.shape(re), np.complex64)
    out.real, out.imag = re, im
    return out


def add32(x, n_re, n_im):
    """complex64 x + (n_re, n_im) per component in float32: the kernel's last step."""
    x = np.asarray(x, np.complex64)
    return to_c64(x.real + np.asarray(n_re, F32), x.imag + np.asarray(n_im, F32))


def fade32(g, x):
    """complex64 g x as the kernel steps it in float32: (g.x x.x - g.y x.y, g.x x.y + g.y x.x)."""
    g, x = np.asarray(g, np.complex64), np.asarray(x, np.complex64)
    return to_c64(g.real * x.real - g.imag * x.imag, g.real * x.imag + g.imag * x.real)


def pilot32(g, p):
    """complex64 g p formed in float64 and rounded once per component: the framing kernel's h p."""
    gr, gi = np.asarray(g).real.astype(F64), np.asarray(g).imag.astype(F64)
    pr, pi = np.asarray(p).real.astype(F64), np.asarray(p).imag.astype(F64)
    return to_c64((gr * pr - gi * pi).astype(F32), (gr * pi + gi * pr).astype(F32))


def block_of(S, coh, variant=None):
    """Gain block of symbol s: s // coh, or ("chunk") taken from the index within the 64-symbol chunk."""
    s = np.arange(S)
    return (s % 64 if variant == "chunk" else s) // coh


# ---- the tolerance ------------------------------------------------------------------------------------
def excess(dev, y_ref, rad):
    """Per component, (|device - y_ref| - ulp32(y_ref) / 2) / rad clipped at 0: what the check compares
    with 4 tau.  rad = 0 (a top u1): 0 where the device is within the half ulp, else +inf.  float64
    [2, ...] (real, imaginary)."""
    dev, y_ref = np.asarray(dev), np.asarray(y_ref, np.complex128)
    rad = np.broadcast_to(np.asarray(rad, F64), y_ref.shape)
    out = []
    for d, y in ((dev.real, y_ref.real), (dev.imag, y_ref.imag)):
        over = np.maximum(np.abs(d.astype(F64) - y) - 0.5 * np.spacing(np.abs(y).astype(F32)).astype(F64), 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(over == 0.0, 0.0, np.where(rad > 0, over / rad, np.inf)))
    return np.stack(out)


def within(dev, y_ref, rad, tau4=None):
    """Whether every component of `dev` is inside the tolerance; NaN is outside."""
    e = excess(dev, y_ref, rad)
    return bool(np.all(e <= (bound() if tau4 is None else tau4)))


def tail_ok(row, dev, y_ref, rad, x):
    """The tail family's check of one sample: a top u1 gives the table point (or los) bit for bit, a top
    u2 gives (rad, 0): the imaginary part untouched; everything under the tolerance."""
    _, _, _, role, v = row
    ok = within(dev, y_ref, rad)
    if v == TOP and role == "u1":
        ok = ok and np.array_equal(dev, x)
    if v == TOP and role == "u2":
        ok = ok and np.array_equal(dev.imag, x.imag)
    return ok


def variance_ok(x, n0):
    """The sample variance per dimension (mean square: the mean is known, 0) within 4 standard errors of
    n0 / 2, relative standard error sqrt(2 / count)."""
    x = np.asarray(x, F64)
    return abs(np.mean(x * x) / (n0 / 2) - 1) <= 4 * np.sqrt(2 / x.size)


def _ratio(n32, n64, rad):
    re, im = n32
    err = np.maximum(np.abs(re.astype(F64) - n64.real), np.abs(im.astype(F64) - n64.imag))
    assert np.all(err[rad == 0] == 0)
    return float(np.max(err[rad > 0] / rad[rad > 0], initial=0.0))


def tail_draw(row):
    """(a, b) uint32 scalars: the two words of a TAILS row's element."""
    dom, off, s, _, _ = row
    a, b = W.stream_words([TAIL_CW0 + off], 2, TAIL_SEED, NOISE if dom == "noise" else FADE)
    return a[0, s], b[0, s]


@functools.lru_cache(maxsize=None)
def tau():
    """The largest |ref32 - ref64| / rad_ref of the float32 restatement over all bulk streams (noise,
    branch noise, pilot noise and gains of every counter case, the fading family's streams) and all
    tail draws, and the largest excess (what is over the half ulp of the final addition, over scat * rad)
    of the gains as the kernel finishes them, los + scat * (...), for every K of the fading family.
    Measured on the host; the bound is 4 times this."""
    worst = 0.0
    sig = F32(0.4)
    for cw0, seed in COUNTERS:
        cw = cws(cw0, B)
        for K in (0.0, 4.0, 1e30):
            for br in range(BULK["R"]):
                worst = max(worst, float(np.max(excess(gains32(cw, 15, seed, K, br), *gains(cw, 15, seed, K, br)))))
        for dom, n in ((NOISE, BULK["S"]), (PILOT, 18), (FADE, 15)):
            for br in range(BULK["R"]):
                s = SQRT_HALF if dom == FADE else sig
                a, b = W.stream_words(cw, n, seed, dom | (br << 16))
                worst = max(worst, _ratio(box_muller32(a, b, s), W.box_muller(a, b, s), radius(a, s)))
    cw = cws(FADING["cw0"], FADING["B"])
    for K in (0.0, 4.0, 1e30):
        for br in range(8):
            g, (ref, rad) = gains32(cw, _S, FADING["seed"], K, br), gains(cw, _S, FADING["seed"], K, br)
            worst = max(worst, float(np.max(excess(g, ref, rad))))
    for dom, s in ((NOISE, sig), (FADE, SQRT_HALF)):
        for br in range(8):
            a, b = W.stream_words(cw, _S, FADING["seed"], dom | (br << 16))
            worst = max(worst, _ratio(box_muller32(a, b, s), W.box_muller(a, b, s), radius(a, s)))
    for row in TAILS:
        a, b = (np.array([v]) for v in tail_draw(row))
        s = sig if row[0] == "noise" else SQRT_HALF
        worst = max(worst, _ratio(box_muller32(a, b, s), W.box_muller(a, b, s), radius(a, s)))
    return worst


def bound():
    return 4.0 * tau()


# ---- mapper ---------------------------------------------------------------------------------------------
def label_table(bps):
    """cons[m] = (m, -m): each output symbol names its own label."""
    m = np.arange(1 << bps, dtype=F32)
    return to_c64(m, -m)


def labels(coded, bps, variant=None):
    """int [B, S]: bps coded bits per label, MSB first, the last symbol zero-padded.  Variants: "lsb"
    labels LSB first, "ones" the last symbol padded with ones."""
    coded = np.asarray(coded)
    rows, n_out = coded.shape
    S = -(-n_out // bps)
    padded = np.pad(coded, ((0, 0), (0, S * bps - n_out)), constant_values=1 if variant == "ones" else 0)
    w = 1 << (np.arange(bps) if variant == "lsb" else np.arange(bps - 1, -1, -1))
    return (padded.reshape(rows, S, bps) * w).sum(-1)


def mapper_census(cases=None):
    """What the mapper shapes reach: {property: set of values}."""
    from modulations_amd import tables as T
    seen = {}
    for n, rate, bps in (MAPPER if cases is None else cases):
        n_out = T.consumed_size(n, T.PUNCTURE_PATTERNS[rate])
        S = -(-n_out // bps)
        for k, v in (("bps", bps), ("n_out % bps == 0", n_out % bps == 0), ("S % 64", S % 64),
                     ("n_out % 32 == 0", n_out % 32 == 0), ("n_out % 256 == 0", n_out % 256 == 0),
                     ("n_out % 4 == 0", n_out % 4 == 0), ("N % 16 == 0", n % 16 == 0),
                     ("2N % 128 == 0", 2 * n % 128 == 0), ("N", n)):
            seen.setdefault(k, set()).add(v)
    return seen


def encode_rows(info, n, rate):
    """oracle.encode of every row with made_up_perm(n): int [rows, n_out]."""
    from modulations_amd import tables as T
    from oracle import oracle as O
    t, G = O.trellis()
    punct = T.PUNCTURE_PATTERNS[rate]
    pm, perm = T.puncture_matrix(punct), made_up_perm(n)
    return np.stack([O.encode(b, n, punct["period"], pm, perm, t, G) for b in info])


# ---- error counts ---------------------------------------------------------------------------------------
def count_batches(n):
    """The error-count family's calls for N = n, each (cw0, decoded int32 [rows, 2N], expected counts):
    row r of the first 2N rows has info bit r flipped (every count 1), in calls of at most COUNT_CHUNK
    rows at the largest cw0; a last call holds an unflipped row, an all-flipped one, a row of 2s and a
    row of -1s (0, 2N, 2N, 2N)."""
    row = 2 * n
    out = []
    for r0 in range(0, row, COUNT_CHUNK):
        rows = min(COUNT_CHUNK, row - r0)
        dec = W.info_bits(cws(COUNT_CW0, rows), n, COUNT_SEED).astype(np.int32)
        dec[np.arange(rows), r0 + np.arange(rows)] ^= 1
        out.append((COUNT_CW0, dec, np.ones(rows, np.int32)))
    dec = W.info_bits(cws(COUNT_CW0, 4), n, COUNT_SEED).astype(np.int32)
    dec[1] ^= 1
    dec[2], dec[3] = 2, -1
    out.append((COUNT_CW0, dec, np.array([0, row, row, row], np.int32)))
    return out


def counter_decoded(cw0, seed, n=BULK["n"]):
    """The counter family's rows for k_count_errors: int32 [B, 2N], the reference info bits of codewords
    cw0 .. cw0 + B - 1 with bit (7 r + 3) % 2N of row r flipped, so every count is 1."""
    dec = W.info_bits(cws(cw0, B), n, seed).astype(np.int32)
    dec[np.arange(B), (7 * np.arange(B) + 3) % (2 * n)] ^= 1
    return dec


def count_errors(dec, cw0, n, seed, skip=None, variant=None):
    """k_count_errors restated: positions where the decoded value differs from the info bit; `skip`
    (a wrong variant) leaves one position out; `variant` "ctr1" / "key1" drops counter or key word 1."""
    info = info_bits(cws(cw0, len(dec)), n, seed, variant).astype(np.int32)
    diff = dec != info
    if skip is not None:
        diff[:, skip] = False
    return diff.sum(1).astype(np.int32)
