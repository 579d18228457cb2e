/* llrq.h -- quantised channel LLRs on a tdec_t handle: int8 and
 * float16 LLR rows into the decoder's plane buffer, and the device quantiser that makes them.
 *
 * Built into libtdec.so beside include/tdec.h, whose conventions hold: device pointers,
 * stream-ordered and allocation free, 0 or a negative TDEC_E* code with the reason in the
 * library's thread-local last-error string, an empty batch a no-op before the pointers
 * are looked at.
 *
 * What a narrow element stands for is exact:
 *   LLRQ_INT8  int8 q is (float)q * step, one float32 multiply with a float32 step > 0;
 *              -128 is accepted and means -128 * step.
 *   LLRQ_F16   IEEE half x is (float)x: infinities and NaN pass through, subnormal halves
 *              are kept.  step must be exactly 1.0f.
 * The plane buffer does not depend on how it was filled (harq.h), so every decoder of
 * tdec.h reads what these calls write; on rows widened by that rule tdec_depuncture_dev
 * and harq_depuncture_acc_dev give the same planes bit for bit.
 *
 * Every call refuses, with TDEC_EINVAL: a step or inv_step that is not finite or is <= 0,
 * step != 1 with LLRQ_F16, an unknown kind, null pointers, negative counts.
 */
#ifndef LLRQ_H
#define LLRQ_H

#include "tdec.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LLRQ_INT8 = 0, LLRQ_F16 = 1 };

/* The decoder llrq_decode_dev runs: the fixed-iteration one, or early stop on the frame, tile
 * or refill decoder (tdec_decode_planes_dev, _es_dev, _es_tile_dev, _es_refill_dev). */
enum { LLRQ_DEC_PLAIN = 0, LLRQ_DEC_ES_FRAME = 1, LLRQ_DEC_ES_TILE = 2, LLRQ_DEC_ES_REFILL = 3 };

/* d_q[i] = (int8) clamp(rintf((float)d_llr[i] * inv_step), -127, 127) for n elements: one
 * float32 multiply by the caller's inv_step > 0 (float32(1) / step, formed on the host), then
 * round to nearest, ties to even.  NaN gives 0 (an erasure), +-inf gives +-127, -0.0 gives 0.
 * d_llr is float, or double with llr_f64 (each value rounded to float first).  Neither
 * pointer needs any alignment.  d_saturated (nullable): one 64-bit device counter to which the
 * number of elements with |x * inv_step| > 127 (the infinities included) is ADDED; it is not
 * touched when null. */
int llrq_quantize_dev(int device, const void *d_llr, int llr_f64, long n, float inv_step, int8_t *d_q,
                      unsigned long long *d_saturated, void *stream);

/* tdec_depuncture_dev on B narrow rows, stride ELEMENTS apart (any stride >= the handle's
 * de-puncture walk, any row base: rows need no alignment).  Punctured and missing components
 * and the lanes past B of the last tile are written as 0.0f.
 * TDEC_ESHORT: stride shorter than the de-puncture walk. */
int llrq_depuncture_dev(tdec_t *h, int B, const void *d_q, int kind, float step, long stride, float *d_planes,
                        void *stream);

/* harq_depuncture_acc_dev on narrow rows: planes += the widened rows, gathered through
 * d_row_of (null: the identity, n_rows == n_slots).  Slots whose entry is outside [0, n_rows)
 * and lanes past n_slots are neither read nor written; a component the pattern does not
 * transmit keeps its bits. */
int llrq_depuncture_acc_dev(tdec_t *h, int n_slots, const void *d_q, int kind, float step, long stride, int n_rows,
                            const int32_t *d_row_of, float *d_planes, void *stream);

/* tdec_decode_batch_dev and its early-stop forms on narrow device rows: llrq_depuncture_dev
 * into the handle's own planes, then the decoder `mode` names, with that form's capacity rules
 * (tdec_reserve / tdec_reserve_es_refill) and errors.  d_n_iter (nullable) is filled by the
 * early-stop modes only. */
int llrq_decode_dev(tdec_t *h, int mode, int B, const void *d_q, int kind, float step, long stride, int32_t *d_bits,
                    double *d_lfinal, int32_t *d_n_iter, void *stream);

/* tdec_decode_batch on narrow HOST rows: the same page-locked staging and double-buffered
 * chunks, but the narrow rows are what is staged and uploaded (1 or 2 bytes per LLR instead
 * of 4); they are widened on the device by llrq_depuncture_dev.  bits (int32) and lfinal
 * (double, nullable) are tdec_decode_batch's. */
int llrq_decode_batch(tdec_t *h, int B, const void *q_host, int kind, float step, long stride, int32_t *bits,
                      double *lfinal);

#ifdef __cplusplus
}
#endif
#endif /* LLRQ_H */
