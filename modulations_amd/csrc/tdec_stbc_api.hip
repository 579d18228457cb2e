// tdec_stbc_api.hip -- transmit diversity (include/stbc.h): the host code of
// the Alamouti combiner (k_stbc_combine, tdec_stbc.hip) and of the generator's 2 x R link
// (k_workload_faded<StbcArgs>, tdec_workload.hip).  Included at the end of tdec_api.hip: it
// needs the handle's internals and the generators' argument helpers.
#include "stbc.h"

// k_stbc_combine over n_pairs = B * S2 / 2 pairs; NV: the noise source (0 nv, 1 nvs[row],
// 2 nvs[row][branch]); vec: 16-byte stores of z and nv_sym; y16: 16-byte loads of y
template <int NV>
static void launch_stbc_combine(bool vec, bool y16, const float2 *y, const float2 *hh, long n_pairs, int R, int S, int coh,
                                int nh, double nv, const double *nvs, float2 *z, double *nv_sym, hipStream_t st) {
    const dim3 grid((unsigned)((n_pairs + BLOCK - 1) / BLOCK));
    if (vec)
        hipLaunchKernelGGL((k_stbc_combine<NV, true>), grid, dim3(BLOCK), 0, st, y, hh, n_pairs, R, S, coh, nh, y16, nv,
                           nvs, z, nv_sym);
    else
        hipLaunchKernelGGL((k_stbc_combine<NV, false>), grid, dim3(BLOCK), 0, st, y, hh, n_pairs, R, S, coh, nh, y16, nv,
                           nvs, z, nv_sym);
}

extern "C" {

int stbc_combine_dev(int device, const float *d_y, const float *d_h, int B, int R, int S, int coh, double noise_var,
                     const double *d_nv_rows, const double *d_nv_branches, float *d_z, double *d_nv_sym, void *stream) {
    if (B < 0 || S < 0 || coh < 2 || coh % 2 || R < 1 || R > 8)
        return fail(TDEC_EINVAL, "bad stbc combine arguments (1 <= R <= 8, coh >= 2 and even)");
    if (d_nv_rows && d_nv_branches) return fail(TDEC_EINVAL, "stbc combine: one noise array at most");
    if (B == 0 || S == 0) return 0;
    if (!d_y || !d_h || !d_z || !d_nv_sym) return fail(TDEC_EINVAL, "bad stbc combine arguments");
    const long S2 = (long)S + (S & 1);
    const long n_pairs = (long)B * (S2 / 2);
    if (S2 > INT32_MAX || (n_pairs + BLOCK - 1) / BLOCK > INT32_MAX)
        return fail(TDEC_EINVAL, "bad stbc combine arguments (batch too long)");
    Guard g(device);
    const int nh = (int)((S2 + coh - 1) / coh);
    // 16-byte stores where a pair's two outputs stay in their row and z and nv_sym allow them
    const bool vec = S % 2 == 0 && (((uintptr_t)d_z | (uintptr_t)d_nv_sym) & 15) == 0;
    const bool y16 = ((uintptr_t)d_y & 15) == 0;
    const float2 *y = reinterpret_cast<const float2 *>(d_y), *hh = reinterpret_cast<const float2 *>(d_h);
    float2 *z = reinterpret_cast<float2 *>(d_z);
    hipStream_t st = (hipStream_t)stream;
    if (d_nv_branches) launch_stbc_combine<2>(vec, y16, y, hh, n_pairs, R, S, coh, nh, 0.0, d_nv_branches, z, d_nv_sym, st);
    else if (d_nv_rows) launch_stbc_combine<1>(vec, y16, y, hh, n_pairs, R, S, coh, nh, 0.0, d_nv_rows, z, d_nv_sym, st);
    else launch_stbc_combine<0>(vec, y16, y, hh, n_pairs, R, S, coh, nh, noise_var, nullptr, z, d_nv_sym, st);
    HIPCHK(hipGetLastError());
    return 0;
}

int stbc_workload_dev(tdec_t *h, int B, int R, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                      double sigma, double rician_k, int coh, float *d_syms, float *d_h, uint8_t *d_info, void *stream) {
    if (!h || B < 0 || cw0 < 0 || R < 1 || R > 8) return fail(TDEC_EINVAL, "bad workload arguments (1 <= R <= 8)");
    if (B == 0) return 0;
    if (coh < 2 || coh % 2) return fail(TDEC_EINVAL, "bad workload arguments (stbc: coh >= 2 and even)");
    WorkloadArgs a;
    StbcArgs f{};
    if (!symbol_args(a, h, B, cw0, seed, cons_iq, M, bps, sigma, d_syms, d_info)) return fail(TDEC_EINVAL, BAD_FADING);
    f.S2 = a.S + (a.S & 1);
    if (!fade_args(f, rician_k, coh, f.S2, d_h)) return fail(TDEC_EINVAL, BAD_FADING);
    f.R = R;
    return workload_launch(h, B, k_workload_faded<StbcArgs>, stream, a, f);
}

}  // extern "C"
