/* sm.h -- spatial multiplexing: two transmit antennas send two
 * different table points in every slot, R receive branches see their sum, and a joint max-log
 * detector over the M^2 hypotheses of a slot writes the decoder's LLR rows.  Also the
 * counter-based workload generator's multiplexed 2 x R link.
 *
 * Built into libtdec.so beside include/tdec.h, whose conventions hold: device pointers,
 * stream-ordered, 0 or a negative TDEC_E* code with the reason in the library's thread-local
 * last-error string, an empty batch a no-op before the pointers are looked at.
 *
 * Slots.  A codeword's S table points are x[0 .. S-1]; T = ceil(S / 2) is the number of slots.
 * Slot m carries x[2m] on antenna 0 and x[2m+1] on antenna 1.  For an odd S antenna 1 is silent
 * in the last slot (it sends 0 + 0j), and the detector searches antenna 0's points only there:
 * the hypothesis set of stream 1 is the single point 0.
 *
 * Channel.  Branch r receives y_r[m] = h_r0 x[2m] + h_r1 x[2m+1] + n, h the EFFECTIVE gains
 * with E|h|^2 = 1/2 (the split of the transmit power is inside the gains, as in stbc.h; no
 * sqrt(2) appears in the detector).  A gain block covers coh >= 1 slots; any value is legal, a
 * slot never straddles a block.
 *
 * The detector, all in f64 without contraction, every f32 input widened first.  For branch r
 * with (h0, h1) its gains of block m / coh, y = y_r[m], and hypothesis (a, b) with table
 * points ca, cb:
 *
 *     u.re = y.re - (h0r*ca.re - h0i*ca.im)      u.im = y.im - (h0r*ca.im + h0i*ca.re)
 *     v.re = u.re - (h1r*cb.re - h1i*cb.im)      v.im = u.im - (h1r*cb.im + h1i*cb.re)
 *     d_r  = v.re*v.re + v.im*v.im
 *
 * every product, difference and sum a rounded f64 value of its own; in the single-stream slot
 * v = u.  Branch r is skipped in slot m if any of its four gain components or either component
 * of y_r[m] is not finite; zero gains are live.
 *
 * Common noise (the scalar noise_var, or d_nv_rows[b]):  D(a, b) = d_0 + d_1 + ... over the
 * live branches in the order r = 0 .. R-1, starting from the first live term, and
 * LLR = (m0 - m1) / nve.  Per-branch noise (d_nv_branches[b][r]): each d_r is divided by its
 * nve_r before the addition, and LLR = m0 - m1.  nve = nv > 0.005 ? nv : 0.005, the reference
 * demapper's floor: a NaN takes the floor, +inf gives zero LLRs.  For bit j (MSB first, as
 * compute_llr) of stream 0, m0 / m1 are the minima of D over all (a, b) with bit j of a equal
 * to 0 / 1; stream 1 likewise over b.  The table's components are at most 1e30 in magnitude (a
 * larger or non-finite one is refused), so with f32 y and h nothing in D can overflow f64: D is
 * finite, never -0 and never NaN, and a minimum does not depend on the order of its operands;
 * only the order inside D is pinned.
 *
 * The written value is sign * (float)clip(LLR, -30, 30), sign = +1 the reference sign (positive
 * for bit 1), -1 the decoder's.  A slot with no live branch is an erasure: all of its LLRs are
 * +0.0f.  If m0 - m1 is NaN, that bit is +0.0f -- a guard only: for the tables that are
 * accepted both minima are finite and the case cannot arise.
 */
#ifndef SM_H
#define SM_H

#include "tdec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_y complex64 [B][R][T], T = ceil(S / 2); d_h complex64 [B][R][2][nh], nh = ceil(T / coh)
 * (antenna a of branch r at [b][r][a]), 1 <= R <= 8; cons: the label-ordered table, M points in
 * host memory (f32 pairs, or f64 pairs when cons_f64, as tdec_demap_dev takes it), M = 2^bps a
 * power of two, 2 <= M <= 64 -> d_llr float32 [B] rows of llr_stride >= S * bps floats, symbol
 * s, bit j at s * bps + j; elements of a row behind S * bps are not written.  Noise: noise_var,
 * or d_nv_rows f64 [B], or d_nv_branches f64 [B][R]; one array at most.  Any B * T is taken: a
 * batch whose B * T * M threads do not fit one launch (2^32) is queued as several, in order.
 * The sizes are checked first: TDEC_EINVAL for a negative B or S, coh < 1, R outside 1 .. 8, M
 * outside 2 .. 64 or not a power of two, llr_stride < S * bps, both noise arrays.  Then B == 0 or
 * S == 0 is a no-op, before any pointer is looked at (cons included).  Then TDEC_EINVAL for a null
 * d_y, d_h, cons or d_llr and for a table component that is not finite or above 1e30 in
 * magnitude.  Nothing is written by a refused call.  (sign: negative is -1, anything else +1.) */
int sm_detect_dev(int device, const float *d_y, const float *d_h, int B, int R, int S, int coh, const void *cons,
                  int cons_f64, int M, double noise_var, const double *d_nv_rows, const double *d_nv_branches, int sign,
                  float *d_llr, long llr_stride, void *stream);

/* The multiplexed 2 x R link of global codewords cw0 .. cw0 + B - 1: the info bits of (seed,
 * cw0 + c) and their labels as in every generator call, shared by the branches, sent as above.
 * d_y complex64 [B][R][T], d_h complex64 [B][R][2][nh], nh = ceil(T / coh), coh >= 1 in slots.
 * Raw gain of antenna 0 to branch b, block j: the branch generator's draw (domain word
 * 0x3C5D | b << 16); of antenna 1: the same draw on the domain word 0x6F8A | b << 16, both as
 * in stbc.h.  The written, effective gain is the raw one times 0.70710678118654752f per
 * component in f32.  Slot m of branch b, s0 = x[2m], s1 = x[2m+1] (0 + 0j for the silent
 * antenna), all f32, no contraction:
 *     re = ((h0r*s0r - h0i*s0i) + (h1r*s1r - h1i*s1i)) + n.re
 *     im = ((h0r*s0i + h0i*s0r) + (h1r*s1i + h1i*s1r)) + n.im
 * n the sample tdec_workload_branches_dev adds at symbol index m of branch b (domain word
 * 0x2B0E | b << 16).  A codeword depends on its global index only.  d_info (nullable) receives
 * the info bits.  TDEC_EINVAL: as tdec_workload_branches_dev. */
int sm_workload_dev(tdec_t *h, int B, int R, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                    double sigma, double rician_k, int coh, float *d_y, float *d_h, uint8_t *d_info, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SM_H */
