// tdec_llrq_api.hip -- quantised channel LLRs (include/llrq.h): the host code of
// the narrow-row de-puncture kernels and the quantiser (tdec_llrq.hip).  Included at the end of
// tdec_api.hip: it needs the handle's internals, decode_batch_dev and host_decode_batch.
#include "llrq.h"

namespace {

// What every call checks of (kind, step) before anything else; the element size, or 0 with the error set.
size_t q_elem_size(int kind, float step) {
    if (kind != LLRQ_INT8 && kind != LLRQ_F16) return fail(TDEC_EINVAL, "unknown LLR kind (LLRQ_INT8 or LLRQ_F16)"), 0;
    if (!std::isfinite(step) || step <= 0.0f) return fail(TDEC_EINVAL, "step must be finite and > 0"), 0;
    if (kind == LLRQ_F16 && step != 1.0f) return fail(TDEC_EINVAL, "float16 rows take no step (step must be 1)"), 0;
    return kind == LLRQ_INT8 ? 1 : 2;
}

// threads of a narrow de-puncture launch: one per (tile, group of the kind's steps, lane)
long q_threads(int rows, int N, int kind) {
    const int steps = kind == LLRQ_INT8 ? q_steps<Q_INT8>() : q_steps<Q_F16>();
    return (long)n_tiles_of(rows) * ((N + steps - 1) / steps) * WAVE;
}

constexpr int QZ_MAX_BLOCKS = 2048;   // the quantiser's grid-stride cap: 8 blocks of 256 per compute unit

}  // namespace

extern "C" {

int llrq_quantize_dev(int device, const void *d_llr, int llr_f64, long n, float inv_step, int8_t *d_q,
                      unsigned long long *d_saturated, void *stream) {
    if (n < 0) return fail(TDEC_EINVAL, "bad quantise arguments");
    if (!std::isfinite(inv_step) || inv_step <= 0.0f) return fail(TDEC_EINVAL, "inv_step must be finite and > 0");
    if (n == 0) return 0;
    if (!d_llr || !d_q) return fail(TDEC_EINVAL, "bad quantise arguments");
    Guard g(device);
    const long work = std::max<long>(n / QZ_VEC, 2 * QZ_VEC);   // vectors, or the head and tail elements
    const dim3 grid((unsigned)std::min<long>((work + BLOCK - 1) / BLOCK, QZ_MAX_BLOCKS));
    if (llr_f64)
        hipLaunchKernelGGL(k_llr_quantize<true>, grid, dim3(BLOCK), 0, (hipStream_t)stream, d_llr, n, inv_step, d_q,
                           d_saturated);
    else
        hipLaunchKernelGGL(k_llr_quantize<false>, grid, dim3(BLOCK), 0, (hipStream_t)stream, d_llr, n, inv_step, d_q,
                           d_saturated);
    HIPCHK(hipGetLastError());
    return 0;
}

int llrq_depuncture_dev(tdec_t *h, int B, const void *d_q, int kind, float step, long stride, float *d_planes,
                        void *stream) {
    if (!h || B < 0) return fail(TDEC_EINVAL, "bad depuncture arguments");
    if (!q_elem_size(kind, step)) return TDEC_EINVAL;
    if (B == 0) return 0;
    if (!d_q || !d_planes) return fail(TDEC_EINVAL, "bad depuncture arguments");
    if (stride < h->llr_len) return fail(TDEC_ESHORT, "llr rows shorter than the de-puncture walk");
    Guard g(h->device);
    const long total = q_threads(B, h->N, kind);
    const dim3 grid((unsigned)((total + BLOCK - 1) / BLOCK));
    if (kind == LLRQ_INT8)
        hipLaunchKernelGGL(k_depuncture_q<Q_INT8>, grid, dim3(BLOCK), 0, (hipStream_t)stream, B, h->N,
                           (const int8_t *)d_q, step, stride, (const int *)h->d_src, d_planes, total);
    else
        hipLaunchKernelGGL(k_depuncture_q<Q_F16>, grid, dim3(BLOCK), 0, (hipStream_t)stream, B, h->N,
                           (const _Float16 *)d_q, step, stride, (const int *)h->d_src, d_planes, total);
    HIPCHK(hipGetLastError());
    return 0;
}

int llrq_depuncture_acc_dev(tdec_t *h, int n_slots, const void *d_q, int kind, float step, long stride, int n_rows,
                            const int32_t *d_row_of, float *d_planes, void *stream) {
    if (!h || n_slots < 0 || n_rows < 0) return fail(TDEC_EINVAL, "bad accumulate arguments");
    if (!q_elem_size(kind, step)) return TDEC_EINVAL;
    if (n_slots == 0) return 0;
    if (!d_q || !d_planes) return fail(TDEC_EINVAL, "bad accumulate arguments");
    if (stride < h->llr_len) return fail(TDEC_ESHORT, "llr rows shorter than the de-puncture walk");
    if (!d_row_of && n_rows != n_slots)
        return fail(TDEC_EINVAL, "bad accumulate arguments (without row_of every slot takes its own row: n_rows == n_slots)");
    Guard g(h->device);
    const long total = q_threads(n_slots, h->N, kind);
    const dim3 grid((unsigned)((total + BLOCK - 1) / BLOCK));
    if (kind == LLRQ_INT8)
        hipLaunchKernelGGL(k_depuncture_acc_q<Q_INT8>, grid, dim3(BLOCK), 0, (hipStream_t)stream, n_slots, h->N,
                           (const int8_t *)d_q, step, stride, n_rows, (const int *)d_row_of, (const int *)h->d_src,
                           d_planes, total);
    else
        hipLaunchKernelGGL(k_depuncture_acc_q<Q_F16>, grid, dim3(BLOCK), 0, (hipStream_t)stream, n_slots, h->N,
                           (const _Float16 *)d_q, step, stride, n_rows, (const int *)d_row_of, (const int *)h->d_src,
                           d_planes, total);
    HIPCHK(hipGetLastError());
    return 0;
}

int llrq_decode_dev(tdec_t *h, int mode, int B, const void *d_q, int kind, float step, long stride, int32_t *d_bits,
                    double *d_lfinal, int32_t *d_n_iter, void *stream) {
    if (!h || B < 0 || mode < LLRQ_DEC_PLAIN || mode > LLRQ_DEC_ES_REFILL) return fail(TDEC_EINVAL, "bad decode arguments");
    const size_t esz = q_elem_size(kind, step);
    if (!esz) return TDEC_EINVAL;
    if (B == 0) return 0;
    if (!d_q || !d_bits) return fail(TDEC_EINVAL, "bad decode arguments");
    if (stride < h->llr_len) return fail(TDEC_ESHORT, "llr rows shorter than the de-puncture walk");
    // each mode's own checks, as the float form of that mode makes them before its de-puncture
    if (mode == LLRQ_DEC_ES_FRAME)
        if (int rc = es_available(h)) return rc;
    if (mode == LLRQ_DEC_ES_REFILL) {
        const int w = std::min(n_tiles_of(B), h->max_waves);
        if (w > h->ws_waves || rf_planes_bytes(h, w) > h->planes_rf.cap)
            return fail(TDEC_ECAPACITY, "workspace too small: call tdec_reserve_es_refill first");
    }
    static const DecodeMode MODES[4] = {DEC_PLAIN, DEC_ES_FRAME, DEC_ES_TILE, DEC_ES_REFILL};
    return decode_batch_dev(h, MODES[mode], B, d_bits, d_lfinal, mode == LLRQ_DEC_PLAIN ? nullptr : d_n_iter, stream,
                            [=](int n, long r0, float *planes) {
                                return llrq_depuncture_dev(h, n, (const char *)d_q + r0 * stride * esz, kind, step, stride,
                                                           planes, stream);
                            });
}

int llrq_decode_batch(tdec_t *h, int B, const void *q_host, int kind, float step, long stride, int32_t *bits,
                      double *lfinal) {
    if (!h || B < 0) return fail(TDEC_EINVAL, "bad decode arguments");
    const size_t esz = q_elem_size(kind, step);
    if (!esz) return TDEC_EINVAL;
    CHECK_ARGS(h, B, q_host, bits, &stride);
    return host_decode_batch(h, B, q_host, esz, stride, bits, lfinal,
                             [=](int n, const void *d_q, int32_t *d_bits, double *d_lf) {
                                 return llrq_decode_dev(h, LLRQ_DEC_PLAIN, n, d_q, kind, step, stride, d_bits, d_lf, nullptr,
                                                        h->stream);
                             });
}

}  // extern "C"
