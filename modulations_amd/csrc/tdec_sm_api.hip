// tdec_sm_api.hip -- spatial multiplexing (include/sm.h): the host code of the
// joint detector (k_sm_detect, tdec_sm.hip) and of the generator's multiplexed 2 x R link
// (k_workload_faded<SmArgs>, tdec_workload.hip).  Included at the end of tdec_api.hip: it needs
// the demapper's table cache and the generators' argument helpers.
#include "sm.h"

static constexpr double SM_MAX_POINT = 1e30;   // include/sm.h: the largest table component taken
static constexpr long SM_MAX_BLOCKS = ((1L << 32) / BLOCK) - 1;   // blocks per launch: below 2^32 threads

// k_sm_detect<M, NV> over n_slots = B * T slots, 64 / M slots per wave, R * 64 * 16 bytes of LDS per wave.
// A slot takes M threads and a launch holds fewer than 2^32 (gridDim.x * BLOCK must fit 32 bits), so a long
// batch goes out as several launches of at most SM_MAX_BLOCKS blocks, each from its first slot on.
template <int M, int NV>
static void launch_sm_detect(const float2 *y, const float2 *hh, const double2 *tab, long n_slots, int R, int S, int T,
                             int coh, int nh, double nv, const double *nvs, float sgn, float *llr, long stride,
                             hipStream_t st) {
    const long per_block = (long)(BLOCK / 64) * (64 / M);
    const size_t lds = (size_t)(BLOCK / 64) * R * 64 * sizeof(double2);
    for (long slot0 = 0; slot0 < n_slots; slot0 += SM_MAX_BLOCKS * per_block) {
        const long blocks = std::min(SM_MAX_BLOCKS, (n_slots - slot0 + per_block - 1) / per_block);
        hipLaunchKernelGGL((k_sm_detect<M, NV>), dim3((unsigned)blocks), dim3(BLOCK), lds, st, y, hh, tab, slot0, n_slots,
                           R, S, T, coh, nh, nv, nvs, sgn, llr, stride);
    }
}

template <int NV, typename... A> static void launch_sm_detect_m(int M, A... a) {
    switch (M) {
    case 2: launch_sm_detect<2, NV>(a...); break;
    case 4: launch_sm_detect<4, NV>(a...); break;
    case 8: launch_sm_detect<8, NV>(a...); break;
    case 16: launch_sm_detect<16, NV>(a...); break;
    case 32: launch_sm_detect<32, NV>(a...); break;
    default: launch_sm_detect<64, NV>(a...); break;
    }
}

extern "C" {

int sm_detect_dev(int device, const float *d_y, const float *d_h, int B, int R, int S, int coh, const void *cons,
                  int cons_f64, int M, double noise_var, const double *d_nv_rows, const double *d_nv_branches, int sign,
                  float *d_llr, long llr_stride, void *stream) {
    if (B < 0 || S < 0 || coh < 1 || R < 1 || R > 8)
        return fail(TDEC_EINVAL, "bad sm detect arguments (1 <= R <= 8, coh >= 1)");
    if (M < 2 || M > 64 || (M & (M - 1))) return fail(TDEC_EINVAL, "sm detect: M must be a power of two, 2 .. 64");
    if (d_nv_rows && d_nv_branches) return fail(TDEC_EINVAL, "sm detect: one noise array at most");
    int bps = 0;
    while ((1 << bps) < M) ++bps;
    if (llr_stride < (long)S * bps) return fail(TDEC_EINVAL, "sm detect: the row stride is below S * bps");
    if (B == 0 || S == 0) return 0;   // an empty batch: a no-op before any pointer is looked at
    if (!d_y || !d_h || !cons || !d_llr) return fail(TDEC_EINVAL, "bad sm detect arguments");
    // |c| <= 1e30 per component: with f32 y and h no product, square or sum of the definition can then
    // overflow f64 (|h c| < 7e68, d_r < 2e138, D / 0.005 < 4e141), so D is finite and never NaN
    for (int i = 0; i < 2 * M; ++i) {
        const double c = cons_f64 ? ((const double *)cons)[i] : (double)((const float *)cons)[i];
        if (!(std::fabs(c) <= SM_MAX_POINT))
            return fail(TDEC_EINVAL, "sm detect: table components must be finite and at most 1e30 in magnitude");
    }
    const int T = (int)(((long)S + 1) / 2);
    const long n_slots = (long)B * T;
    Guard g(device);
    hipStream_t st = (hipStream_t)stream;
    ConsCache *cc = nullptr;
    if (int rc = cached_table(device, cons, cons_f64, M, bps, true, st, &cc)) return rc;
    const double2 *tab = reinterpret_cast<const double2 *>(cc->buf.p);
    const int nh = (T + coh - 1) / coh;
    const float2 *y = reinterpret_cast<const float2 *>(d_y), *hh = reinterpret_cast<const float2 *>(d_h);
    const float sgn = sign < 0 ? -1.0f : 1.0f;
    if (d_nv_branches)
        launch_sm_detect_m<2>(M, y, hh, tab, n_slots, R, S, T, coh, nh, 0.0, d_nv_branches, sgn, d_llr, llr_stride, st);
    else if (d_nv_rows)
        launch_sm_detect_m<1>(M, y, hh, tab, n_slots, R, S, T, coh, nh, 0.0, d_nv_rows, sgn, d_llr, llr_stride, st);
    else
        launch_sm_detect_m<0>(M, y, hh, tab, n_slots, R, S, T, coh, nh, noise_var, (const double *)nullptr, sgn, d_llr,
                              llr_stride, st);
    HIPCHK(hipGetLastError());
    return 0;
}

int sm_workload_dev(tdec_t *h, int B, int R, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                    double sigma, double rician_k, int coh, float *d_y, float *d_h, uint8_t *d_info, void *stream) {
    if (!h || B < 0 || cw0 < 0 || R < 1 || R > 8) return fail(TDEC_EINVAL, "bad workload arguments (1 <= R <= 8)");
    if (B == 0) return 0;
    WorkloadArgs a;
    SmArgs f{};
    if (!symbol_args(a, h, B, cw0, seed, cons_iq, M, bps, sigma, d_y, d_info)) return fail(TDEC_EINVAL, BAD_FADING);
    f.T = (a.S + 1) / 2;
    if (!fade_args(f, rician_k, coh, f.T, d_h)) return fail(TDEC_EINVAL, BAD_FADING);
    f.R = R;
    return workload_launch(h, B, k_workload_faded<SmArgs>, stream, a, f);
}

}  // extern "C"
