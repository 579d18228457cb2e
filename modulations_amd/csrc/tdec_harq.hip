// tdec_harq.hip -- hybrid ARQ (include/harq.h): the host code of the
// soft-combining kernel (k_depuncture_acc, tdec_kernels.hip) and of the generator's
// retransmissions (k_workload_faded<TxArgs>, tdec_workload.hip).  Included at the end of
// tdec_api.hip: it needs the handle's internals and the generators' argument helpers.
#include "harq.h"

extern "C" {

int harq_depuncture_acc_dev(tdec_t *h, int n_slots, const void *d_llr, int llr_f64, long llr_stride, int n_rows,
                            const int32_t *d_row_of, float *d_planes, void *stream) {
    if (!h || n_slots < 0 || n_rows < 0) return fail(TDEC_EINVAL, "bad accumulate arguments");
    if (n_slots == 0) return 0;   // an empty batch is a no-op (every batched entry point)
    if (!d_llr || !d_planes) return fail(TDEC_EINVAL, "bad accumulate arguments");
    if (llr_stride < h->llr_len) return fail(TDEC_ESHORT, "llr rows shorter than the de-puncture walk");
    if (!d_row_of && n_rows != n_slots)
        return fail(TDEC_EINVAL, "bad accumulate arguments (without row_of every slot takes its own row: n_rows == n_slots)");
    Guard g(h->device);
    const long total = (long)n_tiles_of(n_slots) * h->N * WAVE;
    const dim3 grid((unsigned)((total + BLOCK - 1) / BLOCK));
    if (llr_f64)
        hipLaunchKernelGGL(k_depuncture_acc<true>, grid, dim3(BLOCK), 0, (hipStream_t)stream, n_slots, h->N, d_llr,
                           llr_stride, n_rows, (const int *)d_row_of, (const int *)h->d_src, d_planes, total);
    else
        hipLaunchKernelGGL(k_depuncture_acc<false>, grid, dim3(BLOCK), 0, (hipStream_t)stream, n_slots, h->N, d_llr,
                           llr_stride, n_rows, (const int *)d_row_of, (const int *)h->d_src, d_planes, total);
    HIPCHK(hipGetLastError());
    return 0;
}

int harq_workload_tx_dev(tdec_t *h, int B, int tx, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                         double sigma, int fading, double rician_k, int coh, float *d_syms, float *d_h,
                         uint8_t *d_info, void *stream) {
    if (!h || B < 0 || cw0 < 0 || tx < 0 || tx > 65535)
        return fail(TDEC_EINVAL, "bad workload arguments (0 <= tx <= 65535)");
    if (B == 0) return 0;
    WorkloadArgs a;
    TxArgs f{};
    if (!symbol_args(a, h, B, cw0, seed, cons_iq, M, bps, sigma, d_syms, d_info) ||
        (fading && !fade_args(f, rician_k, coh, a.S, d_h)))
        return fail(TDEC_EINVAL, BAD_FADING);
    f.tx = tx;
    f.fade = fading != 0;
    return workload_launch(h, B, k_workload_faded<TxArgs>, stream, a, f);
}

}  // extern "C"
