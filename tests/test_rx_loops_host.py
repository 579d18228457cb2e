"""The case tables of tests/rx_loops.py, checked on the CPU: the restatements against numpy's
own expressions, the conditions the designed inputs must meet (no toleranced trajectory grazes a
discontinuity of its detector, and the long double run decides every step as the float64 one
does), that every wrong variant of the restatement is told from the right one by a named family,
and a census of the detector edges and lane counts the tables reach.  Nothing here is built for
or run on a GPU."""
import numpy as np
import pytest

import rx_loops as X
from modulations_amd import modem as MM

CASES = X.carrier_cases()
EXACT = [n for n, c in CASES.items() if c.exact]
TOLERANCED = [n for n, c in CASES.items() if not c.exact]


# ---------------------------------------------------------------- the restatements ------------
def test_constants_are_the_projects():
    assert (X.CR_BPSK, X.CR_QUAD, X.CR_PSK8) == (MM.CR_BPSK, MM.CR_QUAD, MM.CR_PSK8)
    assert X.ALPHAS == {"sync": 0.03, **{m: v["alpha"] for m, v in MM.SDRModem.MODULATIONS.items()}}
    assert {m: X.ALPHA_KIND[m] for m in MM.SDRModem.MODULATIONS} == \
        {m: MM.SDRModem._detector(m) for m in MM.SDRModem.MODULATIONS}
    assert X.Q == 0.7853981633974483 and X.STRIDE == 1 << 20


def test_step_is_numpys_expressions():
    """One step in complex arithmetic, as the contract writes it, on every exact one-step lane and
    on the 8PSK lanes: s * np.exp(-1j * phase), np.sign, np.round, np.angle."""
    for name in ("onestep", "tiny", "psk8_step"):
        c = CASES[name]
        out, fin = X.carrier_f64(c)
        with np.errstate(all="ignore"):
            o = c.syms[:, 0] * np.exp(-1j * c.ph)
            e0 = o.imag * np.sign(o.real)
            e1 = np.sign(o.real) * o.imag - np.sign(o.imag) * o.real
            p = np.angle(o)
            e2 = np.sin(p - np.round(p / (np.pi / 4)) * (np.pi / 4))
            err = np.select([c.kind == 0, c.kind == 1], [e0, e1], e2)
            freq = c.fr + (c.al * 0.1) * err
            phase = c.ph + (c.al * err + freq)
        assert X.same_bits(out[:, 0], o), name
        assert X.same_bits(fin, np.stack([phase, freq], axis=1)), name
    assert np.sign(-0.0) == 0 and not np.signbit(np.sign(np.float64(-0.0))) and np.isnan(np.sign(np.nan))
    assert np.round(0.5) == 0 and np.round(1.5) == 2 and np.round(-0.5) == 0


def test_unknown_kind_is_nan():
    c = CASES["batch63"]
    kind = c.kind.copy()
    kind[[5, 62]] = (3, -1)
    re, im, fin = X.carrier_run(c.syms, c.ph, c.fr, c.al, kind)
    bad = np.zeros(63, bool)
    bad[[5, 62]] = True
    assert np.isnan(fin[bad]).all() and np.isfinite(fin[~bad]).all()
    assert np.isfinite(re[:, 0]).all() and np.isnan(re[bad, 1:]).all() and np.isfinite(re[~bad]).all()


@pytest.mark.parametrize("k", range(len(X.mix_cases())), ids=[c.name for c in X.mix_cases()])
def test_mixer_table(k):
    c = X.mix_cases()[k]
    sig, dc = X.mix_inputs(c)
    assert sig.dtype == c.dtype and len(sig) == c.n and (dc is None) == (not c.has_dc)
    re, im = X.mix_ref(sig, dc, c.w, X.MIX_FS, c.i0)
    if c.exact:
        th = X.mix_angle(c.n, c.i0, c.w, X.MIX_FS)
        assert not th.any() and np.signbit(th).all() == (c.i0 < 0) and np.signbit(th).any() == (c.i0 < 0)
        if c.i0 >= 0:       # the angle is +0: numpy's own product by 1 + 0j
            assert X.same_bits(X._cplx(re, im), X.mix_numpy_w0(sig, dc))
        assert np.isnan(re).any() == c.special
    else:
        assert np.isfinite(sig.view(sig.real.dtype)).all()
        ld = X.mix_ref(sig, dc, c.w, X.MIX_FS, c.i0, X.LD)
        assert np.all(X.mix_distance(X._cplx(re, im), ld) <= X.mix_bound(sig, dc) / 4)   # the restatement itself
    if c.has_dc:
        assert c.dtype == X.C128 or float(np.float32(dc.real)) != dc.real
        assert not np.array_equal(X.mix_centered(sig, dc), sig.astype(X.C128))


def test_mixer_census():
    cs = X.mix_cases()
    for dt in (X.C64, X.C128):
        for has_dc in (False, True):
            mine = [c for c in cs if c.dtype == dt and c.has_dc == has_dc]
            assert {c.n for c in mine if c.exact} >= set(X.MIX_LENGTHS)
            assert {c.n for c in mine if not c.exact} >= set(X.MIX_LENGTHS)
            assert any(c.special for c in mine)
            assert {c.i0 for c in mine if not c.exact} >= {X.MIX_I0_BIG, X.MIX_I0_NEG, -X.MIX_I0_BIG}
        assert any(c.n == X.MIX_LARGE and c.exact and c.dtype == dt for c in cs)
        assert any(c.n == X.MIX_LARGE and not c.exact and c.dtype == dt for c in cs)
    # only part of the grid takes a second trip, and that part is more than one workgroup
    assert X.BLOCK < X.MIX_LARGE - X.STRIDE < X.STRIDE and X.MIX_I0_BIG > 2 ** 31
    # the special samples: every pair of classes, signs kept
    sig, _ = X.mix_inputs(next(c for c in cs if c.special and c.dtype == X.C64))
    head = sig[:49]
    assert np.isnan(head.real).sum() == 7 and np.isinf(head.imag).sum() == 14
    assert np.sum((head.real == 0) & np.signbit(head.real)) == 7 and np.sum((head.imag == 0) & np.signbit(head.imag)) == 7
    print(f"mixer: {len(cs)} cases, {sum(c.exact for c in cs)} exact")


MIX_MISSES = {"dc_in_f64": "w0-n257-complex64-dc (exact)", "i0_int32": "tone-i0big (toleranced)",
              "angle_regrouped": "tone-i0big (toleranced)"}


@pytest.mark.parametrize("variant", X.MIX_VARIANTS)
def test_mixer_cases_catch_near_misses(variant):
    cs = {c.name: c for c in X.mix_cases()}
    if variant == "dc_in_f64":
        c = cs["w0-n257-complex64-dc"]
        sig, dc = X.mix_inputs(c)
        good, bad = (X._cplx(*X.mix_ref(sig, dc, c.w, X.MIX_FS, c.i0, variant=v)) for v in (None, variant))
        assert not X.same_bits(good, bad), MIX_MISSES[variant]
        return
    for dt in ("complex64", "complex128"):
        c = cs[f"tone-i0big-{dt}-dc"]
        sig, dc = X.mix_inputs(c)
        ld = X.mix_ref(sig, dc, c.w, X.MIX_FS, c.i0, X.LD)
        bad = X._cplx(*X.mix_ref(sig, dc, c.w, X.MIX_FS, c.i0, variant=variant))
        assert np.any(X.mix_distance(bad, ld) > X.mix_bound(sig, dc)), MIX_MISSES[variant]


# ---------------------------------------------------------------- the designed inputs ---------
def test_exact_cases_are_what_they_claim():
    c = CASES["onestep"]
    assert not c.ph.any() and c.syms.shape[1] == 1 and set(c.kind) == {0, 1}
    assert np.all(np.isfinite(c.fr) & np.isfinite(c.al) & (c.fr != 0) & (c.al > 0))
    t = CASES["tiny"]
    assert np.all((np.abs(t.ph) <= 2.0 ** -30) & (t.ph != 0)) and {-1.0, 1.0} == set(np.sign(t.ph))
    assert np.array_equal(np.cos(t.ph), np.ones(256)) and np.array_equal(np.sin(t.ph), t.ph)
    assert np.array_equal(np.sin(t.ph.astype(X.LD)).astype(np.float64), t.ph)       # and far from a rounding boundary
    assert float(np.max(np.abs(np.sin(t.ph.astype(X.LD)) - t.ph) / np.spacing(np.abs(t.ph)))) < 2.0 ** -8
    for name in ("still", "coast"):
        c = CASES[name]
        out, fin = X.carrier_f64(c)
        assert not c.al.any() and not c.ph.any() and list(c.kind) == [0, 1, 2] and c.syms.shape == (3, 300)
        assert X.same_bits(out[:, 0], c.syms[:, 0])
        if name == "still":
            assert X.same_bits(out, c.syms) and X.same_bits(fin, np.zeros((3, 2)))
        else:
            ph = np.zeros(3)
            for _ in range(300):
                ph = ph + c.fr
            assert X.same_bits(fin, np.stack([ph, c.fr], axis=1)) and np.all(np.abs(fin[:, 0]) > 2.9)


def test_nan_case_on_the_restatement():
    clean, dirty = CASES["nan_clean"], CASES["nan"]
    assert clean.syms.shape == (X.CR_BLOCK, 40) and set(clean.kind) == {0, 1, 2}
    (o0, f0), (o1, f1) = X.carrier_f64(clean), X.carrier_f64(dirty)
    hit = np.zeros(X.CR_BLOCK, bool)
    for lane, step, part in X.NAN_AT:
        hit[lane] = True
        assert np.isnan(dirty.syms[lane, step]) and np.isnan(getattr(dirty.syms[lane, step], part.replace("re", "real")
                                                                     .replace("im", "imag")))
        assert X.same_bits(o1[lane, :step], o0[lane, :step])
        assert np.isnan(o1[lane, step:].real).all() and np.isnan(o1[lane, step:].imag).all() and np.isnan(f1[lane]).all()
    assert {k for k in dirty.kind[hit]} == {0, 1, 2}
    assert X.same_bits(o1[~hit], o0[~hit]) and X.same_bits(f1[~hit], f0[~hit]) and np.isfinite(f0).all()


@pytest.mark.parametrize("name", TOLERANCED)
def test_toleranced_streams_keep_clear_of_the_discontinuities(name):
    c = CASES[name]
    (re_l, im_l, fin_l), cpu, bound = X.carrier_refs(name)
    re, im, fin = X.carrier_run(c.syms, c.ph, c.fr, c.al, c.kind)
    assert np.isfinite(c.syms.view(np.float64)).all() and np.all(np.abs(c.syms) > 0.1)
    m = X.margins(re, im, c.syms, c.kind)
    designed = np.zeros(m.shape, bool)
    designed[:, 0] = c.edge0
    assert np.all(m[~designed] > X.MARGIN), (name, float(np.min(m[~designed])))
    a, b = X.sides(re, im, c.kind)
    a_l, b_l = X.sides(re_l, im_l, c.kind)
    cut = (np.broadcast_to(c.kind[:, None], a.shape) == X.CR_PSK8) & (np.abs(a) == 4)     # -pi and +pi: one sector
    assert np.array_equal(np.where(cut, 4, a), np.where(cut, 4, a_l)) and np.array_equal(b, b_l), name
    n = c.syms.shape[1]
    print(f"{name}: float64 against long double: out {float(cpu[0].max()):.3g}, final {float(cpu[1].max()):.3g}; "
          f"bounds: out {float(bound[0].min()):.3g}..{float(bound[0].max()):.3g}, "
          f"final {float(bound[1].min()):.3g}..{float(bound[1].max()):.3g}; "
          f"closest approach to a discontinuity {float(np.min(m[~designed])):.3g}")
    assert float(bound[0].min()) >= X.RTOL * n / X.RTOL_N and np.all(bound[0] >= 16 * cpu[0])
    assert float(bound[0].max()) < 1e-7 and float(bound[1].max()) < 1e-7       # a bound worth the name
    if name == "long":
        assert np.all(np.abs(fin[:, 0]) > 1e4) and n == 4096 and list(c.al) == list(X.ALPHAS.values())
        assert set(c.kind) == {0, 1, 2}
        # locked: the recovered symbols sit on their constellations to the end
        assert np.all(m[:, -200:] > 0.05)
        assert np.all(np.abs(fin[:, 1] - X.LONG_F) < 0.01)
    if name == "psk8_step":
        z = c.syms[-1, 0]
        assert c.edge0.sum() == 1 and c.edge0[-1] and np.angle(z) / (np.pi / 4) == 0.5 and m[-1, 0] == 0
        exact = np.arctan2(X.LD(z.imag), X.LD(z.real))
        assert abs(float((exact - X.LD(np.angle(z))) / X.LD(np.spacing(np.angle(z))))) < 0.05


# ---------------------------------------------------------------- the wrong variants ----------
# variant -> the families that must tell it from the right restatement (exact ones bit for bit)
DETECTS = {
    "alpha_div_10": ("onestep", "tiny"),
    "phase_uses_old_freq": ("onestep", "tiny", "batch", "long"),
    "phase_sum_regrouped": ("tiny",),
    "rotate_by_plus_phase": ("onestep", "tiny", "batch", "long"),
    "sign0_is_1": ("onestep",),
    "round_half_away": ("psk8_step",),
    "quad_terms_swapped": ("onestep", "tiny", "batch", "long"),
    "psk8_step_pi_8": ("psk8_step",),
}


def differs(c, variant):
    out, fin = X.carrier_f64(c, variant)
    if c.exact:
        good = X.carrier_f64(c)
        return not (X.same_bits(out, good[0]) and X.same_bits(fin, good[1]))
    ref, _, bound = X.carrier_refs(c.name)
    d = X.carrier_distance(out, fin, ref, c.syms)
    return bool(np.any(d[0] > bound[0]) or np.any(d[1] > bound[1]))


@pytest.mark.parametrize("variant", X.CARRIER_VARIANTS)
def test_carrier_cases_catch_wrong_variants(variant):
    assert set(DETECTS) == set(X.CARRIER_VARIANTS)
    for family in DETECTS[variant]:
        mine = [c for c in CASES.values() if c.family == family and c.name != "nan"]
        assert mine and all(differs(c, variant) for c in mine), f"{variant} passes the family '{family}'"


def test_regrouping_is_invisible_from_phase_zero():
    """Why the "tiny" family exists: from phase0 = 0 both groupings of the phase sum agree."""
    assert not differs(CASES["onestep"], "phase_sum_regrouped")
    assert not differs(CASES["coast"], "phase_sum_regrouped") and not differs(CASES["still"], "phase_sum_regrouped")


# ---------------------------------------------------------------- census ----------------------
def test_carrier_census():
    c = CASES["onestep"]
    grid = X.onestep_classes()
    assert len(grid) == 98 and len(set(grid)) == 98

    def cls(v):
        return ("nan" if np.isnan(v) else ("+inf" if v > 0 else "-inf") if np.isinf(v) else
                ("-0" if np.signbit(v) else "+0") if v == 0 else "pos" if v > 0 else "neg")
    assert [(int(k), cls(z.real), cls(z.imag)) for k, z in zip(c.kind, c.syms[:98, 0])] == grid
    out, _ = X.carrier_f64(c)
    # from phase0 = 0 the detector sees the sample's own classes where both parts are finite
    fin_lanes = [i for i, (_, a, b) in enumerate(grid) if "inf" not in a + b and "nan" not in a + b]
    assert all(out[i, 0] == c.syms[i, 0] for i in fin_lanes) and len(fin_lanes) == 32
    p = CASES["psk8_step"]
    re, im, _ = X.carrier_run(p.syms, p.ph, p.fr, p.al, p.kind)
    sectors, _ = X.sides(re, im, p.kind)
    lanes = X.psk8_step_lanes()
    assert len(lanes) == 45 and {k for k, _ in lanes} == set(range(-4, 5))
    assert max(abs(d) for _, d in lanes) <= 0.3 * np.pi / 4 + 1e-15
    assert set(sectors[:, 0]) == set(range(-4, 5))
    for i, (k, d) in enumerate(lanes):
        assert (sectors[i, 0] - k) % 8 == 0, (k, d, sectors[i, 0])
    # (-r, +0.0) and (-r, -0.0): the product by (1, -0.0) the contract prescribes gives im = +0.0 for
    # both (re * -0.0 = +0.0 absorbs the sample's own zero), so both reach arctan2 on the +pi side
    for i in (-3, -2):
        assert re[i, 0] < 0 and im[i, 0] == 0 and not np.signbit(im[i, 0]) and sectors[i, 0] == 4
    assert np.signbit(p.syms[-2, 0].imag) and not np.signbit(p.syms[-3, 0].imag)
    counts = sorted(c.syms.shape[0] for c in CASES.values() if c.family == "batch")
    assert counts == [63, 64, 65, 128, 129, 300]
    for c in CASES.values():
        if c.family == "batch":
            assert c.syms.shape[1] == 64 and np.array_equal(c.kind, np.arange(len(c.kind)) % 3)
            assert len(set(c.al)) == len(c.al) and len(set(c.ph)) == len(c.ph) and len(set(c.fr)) == len(c.fr)
    fam = {}
    for c in CASES.values():
        fam[c.family] = fam.get(c.family, 0) + c.syms.shape[0]
    print("carrier streams per family:", fam)
    assert fam == {"onestep": 354, "tiny": 256, "still": 3, "coast": 3, "nan": 128, "psk8_step": 48, "batch": 749,
                   "long": 7}
