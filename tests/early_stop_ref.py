"""The early-stop rule restated in numpy on top of the oracle's SISO.

TEST INFRASTRUCTURE: the reference's decode loop (dvb_rcs2_turbo.py:464-537) --
its de-puncture walk, its two SISOs per iteration (oracle.siso, the pinned
restatement of :116-281), its f64 gathers through perm / inv_perm and its
hard-decision expression -- with the stopping rule between the iterations:

  D_0 = (Lc_A < 0, Lc_B < 0) on the de-punctured f32 channel LLRs;
  iterations t = 1 .. I-1 run with sf = 0.7; after SISO 2 of iteration t,
  D_t = (((f64)Lc + La_t) + Le1_t) < 0 with La_t = Le2_t[inv_perm] (plain `<`:
  NaN and -0.0 decide 0); if D_t == D_{t-1} on all 2N bits, iteration t + 1 is
  the final one (sf = 1.0) and n_iter = t + 1; without a trigger n_iter = I.

Because an iteration at 0.7 does not depend on how many follow, a row's bits and
L_final equal oracle.decode(..., iterations=n_iter) bit for bit
(tests/test_early_stop_rule.py checks exactly that).
"""
import numpy as np

from oracle import oracle as O


def depuncture(llr, n, punct):
    """The walk of :476-487: (Lc_A, Lc_B, Lc_W1, Lc_Y1, Lc_W2, Lc_Y2), float32 [n]."""
    llr = np.asarray(llr, np.float32)
    out = [np.zeros(n, np.float32) for _ in range(6)]
    idx, period = 0, punct["period"]
    for i in range(n):
        p = i % period
        out[0][i] = llr[idx]; idx += 1
        out[1][i] = llr[idx]; idx += 1
        for j, name in enumerate(("W1", "Y1", "W2", "Y2")):
            if punct[name][p]:
                out[2 + j][i] = llr[idx]; idx += 1
    return out


def decode_early_stop(llr, n, punct, iterations, perm, inv_perm, tables, algo=0):
    """One codeword: (bits int32 [2n], L_final f64 [2n], n_iter)."""
    A, B, W1, Y1, W2, Y2 = depuncture(llr, n, punct)
    perm = np.asarray(perm, np.int64)
    inv = np.asarray(inv_perm, np.int64)
    A_int, B_int = A[perm], B[perm]
    laA, laB = np.zeros(n), np.zeros(n)
    d_prev = np.concatenate([A < 0, B < 0])
    stop = False
    for it in range(iterations):
        last = stop or it == iterations - 1
        sf = 1.0 if last else 0.7
        le1A, le1B = O.siso(A, B, W1, Y1, laA, laB, tables, sf, algo)
        le2A, le2B = O.siso(A_int, B_int, W2, Y2, le1A[perm], le1B[perm], tables, sf, algo)
        laA, laB = le2A[inv], le2B[inv]
        with np.errstate(invalid="ignore"):
            LA = (A.astype(np.float64) + laA) + le1A
            LB = (B.astype(np.float64) + laB) + le1B
            d = np.concatenate([LA < 0, LB < 0])
        if last:
            n_iter = it + 1
            break
        stop = bool(np.array_equal(d, d_prev))
        d_prev = d
    bits = np.zeros(2 * n, np.int32)
    bits[0::2] = LA < 0
    bits[1::2] = LB < 0
    lf = np.zeros(2 * n)
    lf[0::2] = LA
    lf[1::2] = LB
    return bits, lf, n_iter


def decode_early_stop_batch(llr, n, punct, iterations, perm, inv_perm, tables, algo=0):
    """Rows of llr: (bits [B, 2n], L_final [B, 2n], n_iter int32 [B])."""
    rows = [decode_early_stop(r, n, punct, iterations, perm, inv_perm, tables, algo) for r in np.asarray(llr)]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.array([r[2] for r in rows], np.int32))


def bpsk_channel(coded, k_info, rng, ebn0_db):
    """BPSK LLRs 2y / sigma^2 (decoder sign: bit 0 -> +1) of the codewords `coded`
    [B, n] over AWGN at Eb/N0 = ebn0_db (a number, or one value per row [B]):
    float32 [B, n]."""
    r = k_info / coded.shape[1]
    if not np.isscalar(ebn0_db):
        ebn0_db = np.asarray(ebn0_db, np.float64)[:, None]
    sigma2 = 1.0 / (2.0 * r * 10.0 ** (ebn0_db / 10.0))
    y = (1.0 - 2.0 * coded) + rng.standard_normal(coded.shape) * np.sqrt(sigma2)
    return (2.0 * y / sigma2).astype(np.float32)


def bpsk_llrs(codec, rng, B, ebn0_db):
    """bpsk_channel of B random codewords of `codec` at Eb/N0 = ebn0_db:
    (info bits [B, 2N], float32 llr [B, n_coded])."""
    info = rng.integers(0, 2, (B, codec.k_info))
    coded = codec.encode_batch(info)
    return info, bpsk_channel(coded, codec.k_info, rng, ebn0_db)
