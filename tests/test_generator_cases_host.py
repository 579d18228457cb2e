"""The workload generator's case tables (tests/generator_cases.py) do what they claim, on the host:

* the corrected restatements: uniform24 is the kernel's float32 expression (1.0 at the top draw, where
  the float64 form gives 1 - 2^-25), the shared stream words equal the per-file forms they replaced;
* every row of the tail table is recomputed from its counter, and the table holds a top and a bottom
  draw of each uniform in each domain;
* the census of the mapper shapes reaches every branch the issue names, both ways;
* the float32 restatement passes every family's check, and each wrong variant is rejected by the
  family named for it, under that family's tolerance;
* tau, the restatement's own distance to the float64 reference, is what the docstrings record.

The "device" here is the float32 restatement (generator_cases.box_muller32 and friends), right or wrong
in one named way; tests/test_gpu_generator.py runs the same checks on the kernels."""
import numpy as np
import pytest

import fading_ref as F
import generator_cases as G
import pilot_csi_ref as P
from oracle import workload_ref as W

F32, F64 = np.float32, np.float64
SIG = F32(0.4)


# ---- the restatements -----------------------------------------------------------------------------------
def test_uniform24_is_the_float32_expression():
    x = np.array([0, 255, 256, (2 ** 23 - 1) << 8, 2 ** 31, (2 ** 23 + 1) << 8, (G.TOP - 1) << 8, G.TOP << 8, 2 ** 32 - 1],
                 np.uint32)
    u = W.uniform24(x)
    assert u.dtype == F64 and np.all(u > 0) and np.all(u <= 1)
    assert u[0] == u[1] == 2.0 ** -25 and u[2] == 1.5 * 2.0 ** -24
    assert u[3] == (2 ** 23 - 0.5) * 2.0 ** -24             # the last draw whose + 0.5 is representable
    assert u[4] == 0.5 and u[5] == (2 ** 23 + 2) * 2.0 ** -24   # 2^23 + 1.5 rounds to even
    assert u[6] == (2 ** 24 - 2) * 2.0 ** -24 and u[7] == u[8] == 1.0
    assert ((x[7] >> 8).astype(F64) + 0.5) * 2.0 ** -24 == 1 - 2.0 ** -25   # what the files said before


def test_sincospi_is_exact_at_the_quarter_turns():
    sn, cs = W.sincospi(np.array([0.0, 0.5, 1.0, 1.5, 2.0]))
    assert sn.tolist() == [0, 1, 0, -1, 0] and cs.tolist() == [1, 0, -1, 0, 1]
    t = np.linspace(0, 2, 4001)
    sn, cs = W.sincospi(t)
    assert np.max(np.abs(sn - np.sin(np.pi * t))) < 1e-15 and np.max(np.abs(cs - np.cos(np.pi * t))) < 1e-15


def test_shared_words_equal_the_variant_free_forms():
    cw = G.cws(2 ** 40 + 5, 7)
    for dom in (G.NOISE, G.FADE | (2 << 16), G.PILOT):
        for got, want in zip(G.words(cw, 9, G.SEEDS[1], dom), W.stream_words(cw, 9, G.SEEDS[1], dom)):
            assert np.array_equal(got, want)
    # branch 0 of each stream is the untagged one; the branches differ
    assert np.array_equal(W.awgn(cw, 9, 5, 0.3), W.awgn(cw, 9, 5, 0.3, branch=0))
    assert not np.array_equal(W.awgn(cw, 9, 5, 0.3), W.awgn(cw, 9, 5, 0.3, branch=1))
    assert not np.array_equal(P.pilot_noise(cw, 9, 5, 0.3), W.awgn(cw, 9, 5, 0.3))
    assert not np.array_equal(P.pilot_noise(cw, 9, 5, 0.3), P.pilot_noise(cw, 9, 5, 0.3, branch=1))
    # sigma is the device's float32
    assert np.array_equal(W.awgn(cw, 9, 5, 0.3), W.awgn(cw, 9, 5, F64(F32(0.3))))
    import mrc_ref as MR
    g = MR.gains(cw, 3, 5, 11, 4.0)
    assert g.shape == (7, 3, 5) and np.array_equal(g[:, 0], F.gains(cw, 5, 11, 4.0))
    assert np.array_equal(g[:, 2], F.gains(cw, 5, 11, 4.0, branch=2))


def test_tau_is_what_the_docstrings_record():
    """The float32 restatement's worst |ref32 - ref64| / rad over all bulk and tail cases.  The bound on
    the device is 4 times this.  2.25e-7: 3.8 float32 epsilons for six roundings; the gains' last two
    steps (scat *, los +) are in it and do not raise it.  Pinned to the recorded figure: a restatement
    that moved it would move the device's bound with it."""
    t = G.tau()
    print("tau of the float32 restatement", t, "bound", G.bound())
    assert 2.0e-7 < t < 2.5e-7 and G.bound() == 4 * t


# ---- tail table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", G.TAILS, ids=G.TAIL_IDS)
def test_tail_rows_are_the_draws_they_name(row):
    dom, off, s, role, v = row
    a, b = G.tail_draw(row)
    assert int((a if role == "u1" else b) >> 8) == v
    assert v < 4 or v >= 2 ** 24 - 4
    assert G.TAIL_CW0 >= 2 ** 32 and off >= G.TAIL_LANE and s in (0, 1)


def test_tail_table_covers_both_ends_of_both_uniforms_in_both_domains():
    for dom in ("noise", "gain"):
        for role in ("u1", "u2"):
            vs = [v for d, _, _, r, v in G.TAILS if d == dom and r == role]
            assert G.TOP in vs and any(v < 4 for v in vs), (dom, role)
    assert {s for _, _, s, _, _ in G.TAILS} == {0, 1}


def _tail_device(row, variant=None):
    """(device sample complex64 [1], y_ref, rad, x) of a tail row from the float32 restatement."""
    a, b = (np.array([v]) for v in G.tail_draw(row))
    if row[0] == "noise":
        x = np.array([0.9486833 - 0.31622776j], np.complex64)
        dev = G.add32(x, *G.box_muller32(a, b, SIG, variant))
        return dev, x.astype(np.complex128) + W.box_muller(a, b, SIG), G.radius(a, SIG), x
    los, scat = F.los_scat(G.TAIL_K)
    re, im = G.box_muller32(a, b, G.SQRT_HALF, variant)
    dev = G.to_c64(F32(los) + F32(scat) * re, F32(scat) * im)
    x = np.array([los], np.complex64)
    return dev, los + scat * W.box_muller(a, b, G.SQRT_HALF), scat * G.radius(a, G.SQRT_HALF), x


@pytest.mark.parametrize("row", G.TAILS, ids=G.TAIL_IDS)
def test_tail_rows_pass_and_reject_their_variants(row):
    _, _, _, role, v = row
    assert G.tail_ok(row, *_tail_device(row))
    if role == "u1" and v < 4:
        assert not G.tail_ok(row, *_tail_device(row, "nohalf"))         # u without the + 0.5
    if role == "u1" and v >= 2 ** 24 - 4:
        assert not G.tail_ok(row, *_tail_device(row, "u64"))            # u formed in float64
    if role == "u2" and v == G.TOP:
        assert not G.tail_ok(row, *_tail_device(row, "u64"))            # the angle 2 pi (1 - 2^-25): sine not 0


# ---- counter family and bulk ------------------------------------------------------------------------------
def _bulk_ok(cw0, seed, variant, S=G.BULK["S"], dom=G.NOISE, branch=0):
    cw = G.cws(cw0, G.B)
    ref, rad = G.noise(cw, S, seed, SIG, dom, branch)
    x = np.full((G.B, S), 0.9486833 + 0.31622776j, np.complex64)
    dev = G.add32(x, *G.noise32(cw, S, seed, SIG, dom, branch, variant))
    return G.within(dev, x.astype(np.complex128) + ref, rad)


@pytest.mark.parametrize("cw0,seed", G.COUNTERS, ids=G.COUNTER_IDS)
def test_counter_cases_pass_on_every_stream(cw0, seed):
    cw = G.cws(cw0, G.B)
    assert int(cw[-1]) == cw0 + G.B - 1 < 2 ** 63
    for dom in (G.NOISE, G.PILOT, G.NOISE | (2 << 16)):
        assert _bulk_ok(cw0, seed, None, dom=dom)
    for K in (0.0, 4.0, 1e30):
        ref, rad = G.gains(cw, 15, seed, K, branch=1)
        assert G.within(G.gains32(cw, 15, seed, K, branch=1), ref, rad)
    # error counts: one flipped bit per row, each row another position; the unflipped rows count 0
    n = G.BULK["n"]
    dec = G.counter_decoded(cw0, seed)
    info = W.info_bits(cw, n, seed).astype(np.int32)
    assert np.array_equal((dec != info).sum(1), np.ones(G.B)) and len(set(np.nonzero(dec != info)[1])) == 2 * n
    assert np.array_equal(G.count_errors(dec, cw0, n, seed), np.ones(G.B, np.int32))
    assert not G.count_errors(info, cw0, n, seed).any()


def test_counter_family_rejects_dropped_upper_words():
    carry = G.CW0S[1]
    assert carry < 2 ** 32 <= carry + G.B - 1                       # the carry falls inside tile 0
    for variant, differs in (("ctr1", lambda cw0, seed: cw0 + G.B > 2 ** 32), ("key1", lambda cw0, seed: seed >= 2 ** 32)):
        hit = 0
        for cw0, seed in G.COUNTERS:
            cw = G.cws(cw0, G.B)
            same_bits = np.array_equal(G.info_bits(cw, 48, seed, variant), W.info_bits(cw, 48, seed))
            assert same_bits == (not differs(cw0, seed)) == _bulk_ok(cw0, seed, variant)
            # k_count_errors with the word dropped: wrong counts on the flipped rows and on the clean ones
            dec, info = G.counter_decoded(cw0, seed), W.info_bits(cw, 48, seed).astype(np.int32)
            assert np.array_equal(G.count_errors(dec, cw0, 48, seed, variant=variant), np.ones(G.B)) == same_bits
            assert (not G.count_errors(info, cw0, 48, seed, variant=variant).any()) == same_bits
            for dom in (G.FADE, G.PILOT, P.CFO_DOMAIN):
                same = np.array_equal(G.words(cw, 6, seed, dom, variant)[0], G.words(cw, 6, seed, dom)[0])
                assert same == same_bits
            hit += not same_bits
        assert hit >= 6, variant
    # with the carry inside a tile, rows before it agree and rows behind it do not
    cw = G.cws(carry, G.B)
    same = (G.info_bits(cw, 48, G.SEEDS[0], "ctr1") == W.info_bits(cw, 48, G.SEEDS[0])).all(1)
    assert same[:40].all() and not same[40:].any()


@pytest.mark.parametrize("variant", ["s", "swap", "sincos"])
def test_bulk_rejects(variant):
    for cw0, seed in G.COUNTERS:
        assert not _bulk_ok(cw0, seed, variant)
    if variant == "swap":                                              # odd S: the last symbol alone tells
        cw = G.cws(G.CW0S[2], G.B)
        S = G.FADING["S"]
        a, b = G.words(cw, S, G.SEEDS[1], G.NOISE, "swap")
        ra, rb = W.stream_words(cw, S, G.SEEDS[1], G.NOISE)
        assert S % 2 == 1 and not np.any(a[:, -1] == ra[:, -1]) and not np.any(b[:, -1] == rb[:, -1])


def test_variance_check_accepts_the_restatement_and_rejects_sqrt_n0():
    from modulations_amd import demap as D
    from modulations_amd.workload import noise_n0
    v = G.VARIANCE
    cw = G.cws(v["cw0"], G.B)
    for mod, m in D.MODULATIONS.items():
        bps = m["bps"]
        S = -(-6 * v["n"] // bps)
        n0 = noise_n0(D.constellation(mod), 1 / 3, bps, v["ebn0"])
        for sigma, ok in ((np.sqrt(n0 / 2), True), (np.sqrt(n0), False)):
            re, im = G.noise32(cw, S, v["seed"], sigma)
            assert G.variance_ok(np.concatenate([re.ravel(), im.ravel()]), n0) == ok, mod


# ---- frame family -----------------------------------------------------------------------------------------
def _frame_ok(cw0, seed, R, variant):
    """Pilots float32(h p) + pilot noise, branch by branch, from the float32 restatement."""
    plen, dlen, S = G.FRAME["plen"], G.FRAME["dlen"], G.BULK["S"]
    n_p = (P.n_segments(S, dlen) + 1) * plen
    cw = G.cws(cw0, G.B)
    p = P.default_pilots(n_p)
    ok = True
    for b in range(R):
        h = G.gains32(cw, 1, seed, 4.0, b)                              # any gain: one per row
        hp = G.pilot32(h, p[None, :])
        dom, tag = (G.NOISE if variant == "noise-domain" else G.PILOT), (0 if variant == "no-tag" else b)
        dev = G.add32(hp, *G.noise32(cw, n_p, seed, SIG, dom, tag))
        ref, rad = G.noise(cw, n_p, seed, SIG, G.PILOT, b)
        assert np.array_equal(ref, P.pilot_noise(cw, n_p, seed, SIG, b))
        ok = ok and G.within(dev, hp.astype(np.complex128) + ref, rad)
    return ok


@pytest.mark.parametrize("cw0,seed", G.COUNTERS, ids=G.COUNTER_IDS)
def test_frame_family_passes_and_rejects(cw0, seed):
    assert G.FRAME["plen"] % 2 == 1 and G.BULK["S"] % G.FRAME["dlen"] not in (0, G.FRAME["dlen"])
    for R in (1, 3):
        assert _frame_ok(cw0, seed, R, None)
        assert not _frame_ok(cw0, seed, R, "noise-domain")
    assert _frame_ok(cw0, seed, 1, "no-tag") and not _frame_ok(cw0, seed, 3, "no-tag")


# ---- fading family ----------------------------------------------------------------------------------------
def _fading_ok(K, coh, R, variant):
    f = G.FADING
    S, cw = f["S"], G.cws(f["cw0"], f["B"])
    nh = -(-S // coh)
    x = np.exp(2j * np.pi * (np.arange(S) % 8) / 8).astype(np.complex64)[None, :]
    ok = True
    for b in range(R):
        g = G.gains32(cw, nh, f["seed"], K, b)
        ref, rad = G.gains(cw, nh, f["seed"], K, b)
        ok = ok and G.within(g, ref, rad)
        clean = G.fade32(g[:, G.block_of(S, coh, variant)], x)
        dev = G.add32(clean, *G.noise32(cw, S, f["seed"], SIG, G.NOISE, b))
        want = G.fade32(g[:, G.block_of(S, coh)], x)
        n_ref, n_rad = G.noise(cw, S, f["seed"], SIG, G.NOISE, b)
        ok = ok and G.within(dev, want.astype(np.complex128) + n_ref, n_rad)
    return ok


@pytest.mark.parametrize("K,coh,R", [(K, coh, 1) for K, coh in G.FADING_ONE] + G.FADING_BRANCHES)
def test_fading_family_passes_and_rejects_the_chunk_local_block_index(K, coh, R):
    S = G.FADING["S"]
    assert S % 2 == 1 and S > 65
    assert _fading_ok(K, coh, R, None)
    if coh in (63, 65) and K < 1e30:
        assert not _fading_ok(K, coh, R, "chunk")


def test_fading_family_covers_what_it_names():
    S = G.FADING["S"]
    assert {c for _, c in G.FADING_ONE} == {1, 63, 65, S, S + 1} and {k for k, _ in G.FADING_ONE} == {0.0, 4.0, 1e30}
    assert {r for _, _, r in G.FADING_BRANCHES} == {1, 3, 8}
    assert {c for _, c, _ in G.FADING_BRANCHES} >= {1, 63, 65, S, S + 1}
    assert F.los_scat(1e30) == (1.0, F64(F32(1e-15)))


# ---- mapper family ----------------------------------------------------------------------------------------
def test_mapper_census():
    c = G.mapper_census()
    assert c["bps"] == set(range(1, 9))
    for k in ("n_out % bps == 0", "n_out % 32 == 0", "n_out % 256 == 0", "n_out % 4 == 0", "N % 16 == 0", "2N % 128 == 0"):
        assert c[k] == {True, False}, k
    assert c["S % 64"] >= {0, 1, 63} and c["N"] >= {4, 1024}
    assert all(n % 4 == 0 and n <= 1024 for n, _, _ in G.MAPPER) and G.MAPPER_B > 64


@pytest.mark.parametrize("n,rate,bps", G.MAPPER, ids=G.MAPPER_IDS)
def test_mapper_cases_reject_their_variants(n, rate, bps):
    info = W.info_bits(G.cws(G.CW0S[2], 5), n, G.SEEDS[1])
    coded = G.encode_rows(info, n, rate)
    want = G.labels(coded, bps)
    assert want.shape == (5, -(-coded.shape[1] // bps)) and want.max() < (1 << bps)
    tab = G.label_table(bps)
    assert np.array_equal(tab[want].real, want) and np.array_equal(tab[want].imag, -want)
    if bps > 1:
        assert not np.array_equal(G.labels(coded, bps, "lsb"), want)
    if coded.shape[1] % bps:
        ones = G.labels(coded, bps, "ones")
        assert np.array_equal(ones[:, :-1], want[:, :-1]) and np.all(ones[:, -1] != want[:, -1])


# ---- error-count family -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.COUNT_N)
def test_count_batches_flip_every_position_once(n):
    row = 2 * n
    batches = G.count_batches(n)
    flipped = []
    for cw0, dec, want in batches:
        assert cw0 + len(dec) < 2 ** 63 and dec.dtype == np.int32 and dec.shape[1] == row
        assert np.array_equal(G.count_errors(dec, cw0, n, G.COUNT_SEED), want)
    for cw0, dec, want in batches[:-1]:
        info = W.info_bits(G.cws(cw0, len(dec)), n, G.COUNT_SEED)
        r, c = np.nonzero(dec != info)
        assert np.array_equal(r, np.arange(len(dec)))
        flipped += c.tolist()
    assert flipped == list(range(row))
    # a skipped position shows in the row that flips it, wherever it is
    for skip in (0, row - 1, row // 2):
        assert any(not np.array_equal(G.count_errors(dec, cw0, n, G.COUNT_SEED, skip=skip), want)
                   for cw0, dec, want in batches[:-1])
    assert batches[-1][2].tolist() == [0, row, row, row]
