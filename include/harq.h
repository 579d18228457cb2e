/* harq.h -- hybrid ARQ on a tdec_t handle: soft combining of a
 * retransmission into the decoder's plane buffer, and the retransmissions of the
 * counter-based workload generator.
 *
 * Built into libtdec.so beside include/tdec.h, whose conventions hold: device pointers,
 * stream-ordered and allocation free, 0 or a negative TDEC_E* code with the reason in the
 * library's thread-local last-error string, an empty batch a no-op before the pointers
 * are looked at.
 *
 * The plane buffer (its size for a slot count comes from the handle) does not depend on
 * the puncture pattern: per 64-codeword tile, [N][64] float4 {A, B, W1, Y1} followed by
 * [N][64] float2 {W2, Y2}.  Handles of one N with different patterns -- a rate-3/4 first
 * transmission, then the redundancy versions that carry the parity it left out -- therefore
 * fill the same planes, and any decoder of a handle of that N reads them.
 */
#ifndef HARQ_H
#define HARQ_H

#include "tdec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* planes += de-punctured LLR rows of the handle's pattern.
 *
 * Plane slot c (0 <= c < n_slots) takes LLR row d_row_of[c] of the n_rows rows at d_llr
 * (llr_stride elements apart; float, or double with llr_f64, each value rounded to float
 * first).  A null d_row_of is the identity and needs n_rows == n_slots.  An entry outside
 * [0, n_rows), -1 by convention, means no retransmission for that slot: its 24 bytes per
 * trellis step are neither read nor written.
 * For a selected slot every component the pattern transmits at a step becomes
 * plane + llr, one float add; a component it does not transmit keeps its bits.
 * The first transmission is written by the de-puncture or a plane demapper of tdec.h;
 * combinations take effect in the order of the calls on the stream.
 * TDEC_EINVAL: null handle, negative counts, null d_llr / d_planes with n_slots > 0, null
 * d_row_of with n_rows != n_slots.  TDEC_ESHORT: llr_stride shorter than the handle's
 * de-puncture walk. */
int harq_depuncture_acc_dev(tdec_t *h, int n_slots, const void *d_llr, int llr_f64, long llr_stride, int n_rows,
                            const int32_t *d_row_of, float *d_planes, void *stream);

/* Transmission tx (0 .. 65535) of global codewords cw0 .. cw0 + B - 1: the info bits of
 * (seed, cw0 + c) as in every generator call, encoded with the handle's pattern, noise and
 * gains drawn with tx in the upper 16 bits of the counter's domain word.  fading = 0:
 * symbols x + n (d_h, rician_k and coh are not looked at); tx = 0 is then the plain
 * generator's output bit for bit.  fading != 0: h x + n with the gains written to d_h
 * [B][ceil(S / coh)]; tx = 0 is the fading generator's output, tx = b branch b of the
 * branch generator's.  d_info (nullable) receives the info bits. */
int harq_workload_tx_dev(tdec_t *h, int B, int tx, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                         double sigma, int fading, double rician_k, int coh, float *d_syms, float *d_h,
                         uint8_t *d_info, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HARQ_H */
