// tdec_sm.hip -- spatial multiplexing (include/sm.h): the 2 x R joint max-log
// detector.  The generator's side is the SmArgs branch of tdec_workload.hip.
//
// k_sm_detect<M, NV>: y [B][R][T] complex64 through the gains h [B][R][2][nh] and the
// label-ordered f64 table into float32 LLR rows, all in f64, no contraction, the terms and the
// order of their additions include/sm.h's.  NV: the noise source (0 nv, 1 nvs[row],
// 2 nvs[row][branch]), as k_stbc_combine's.
//
// Mapping.  The M values of a (stream 0's label) lie on M consecutive lanes, so a wave holds
// 64 / M consecutive slots of the flat [B][T] slot order and a block of BLOCK threads 4 waves'.
// Each lane forms, once per slot and branch, what depends on one label only:
//   u_r(a) = y_r - h_r0 c_a     in registers (the r loop is unrolled over the 8 legal branches
//                               and left by a uniform branch at R: no indexed register array)
//   p_r(b) = h_r1 c_b, b = the lane's own label, into the wave's LDS strip [R][64]
// each a separately rounded f64 value of the definition, so forming it once changes no
// rounding.  Then every lane loops over b: v = u_r(a) - p_r(b) (an LDS read that the M lanes of
// a slot share), d_r = v.re^2 + v.im^2, D = d_0 + d_1 + ...
//
// A dead branch (a non-finite gain or y) and a lane past the last slot stage u = p = 0: their
// d_r is +0.0, and since D >= +0.0 always (a sum of squares, never -0, never NaN: f32 inputs
// cannot overflow f64 here), D + 0.0 == D and 0.0 + d == d bit for bit: skipping the branch
// and "starting from the first live term" are what the plain sum from r = 0 gives.  In the
// single-stream slot p = 0 likewise and every b gives the same D = D(a): v = u.
//
// Minima.  b's label bits are compile-time: the loop is unrolled fully for M <= 16 and in
// blocks of 16 above, so a hypothesis costs one v_min per low label bit (plus one block minimum
// for M > 16, folded into the high bits' minima and into min_b D once per block, on a uniform
// branch).  Stream 1's 2 bps running minima are then reduced over the slot's M lanes, stream
// 0's are reductions of min_b D(a, b) selected by the lane's own label bits, both by xor
// butterflies, after which every lane of the slot holds all of them; lane i < 2 bps (bps in the
// single-stream slot) forms and writes LLR i, so a wave's stores are contiguous within a row.
// LDS: R * 64 * 16 bytes per wave (dynamic); one barrier, between staging and search.
#include <hip/hip_runtime.h>

namespace tdec {

constexpr int SM_MAX_R = 8;
constexpr int SM_UNROLL = 16;                 // hypotheses of b per unrolled block

template <int M> struct SmBits {
    static constexpr int value = 1 + SmBits<M / 2>::value;
};
template <> struct SmBits<1> {
    static constexpr int value = 0;
};

__device__ __forceinline__ double sm_min(double a, double b) { return __builtin_fmin(a, b); }

template <int W>
__device__ __forceinline__ double sm_group_min(double v) {
#pragma unroll
    for (int o = 1; o < W; o <<= 1) v = sm_min(v, __shfl_xor(v, o));
    return v;
}

// n_slots = B * T; the launch covers the slots from slot0 on (a launch holds fewer than 2^32 threads, so the
// host splits a long batch); nvs: [B] (NV 1) or [B][R] (NV 2); llr rows of `stride` floats
template <int M, int NV>
__global__ __launch_bounds__(BLOCK) void k_sm_detect(const float2 *y, const float2 *h, const double2 *tab, long slot0, long n_slots,
                                                    int R, int S, int T, int coh, int nh, double nv, const double *nvs,
                                                    float sgn, float *llr, long stride) {
    constexpr int BPS = SmBits<M>::value, UB = M < SM_UNROLL ? M : SM_UNROLL, LB = SmBits<UB>::value;
    extern __shared__ double2 sm_p[];         // [waves][R][64]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int a = lane & (M - 1), sl = lane / M;
    const long g = slot0 + ((long)blockIdx.x * (BLOCK / 64) + w) * (64 / M) + sl;
    const bool in = g < n_slots;
    const long row = in ? g / T : 0;
    const int m = in ? (int)(g - row * T) : 0;
    const bool two = 2 * m + 1 < S;           // antenna 1 sends in this slot
    double2 *pw = sm_p + (long)w * R * 64;
    const double2 c = tab[a];
    const float2 *yb = y + row * R * T + m, *hb = h + row * R * 2 * nh + m / coh;
    double ur[SM_MAX_R], ui[SM_MAX_R], nver[SM_MAX_R];
    int n_live = 0;
#pragma unroll
    for (int r = 0; r < SM_MAX_R; ++r) {
        if (r >= R) break;
        const float2 yy = yb[(long)r * T], h0 = hb[(2 * r) * (long)nh], h1 = hb[(2 * r + 1) * (long)nh];
        const bool live = in && fabsf(yy.x) < INFINITY && fabsf(yy.y) < INFINITY && fabsf(h0.x) < INFINITY &&
                          fabsf(h0.y) < INFINITY && fabsf(h1.x) < INFINITY && fabsf(h1.y) < INFINITY;
        const double h0r = (double)h0.x, h0i = (double)h0.y, h1r = (double)h1.x, h1i = (double)h1.y;
        const double u_re = (double)yy.x - (h0r * c.x - h0i * c.y), u_im = (double)yy.y - (h0r * c.y + h0i * c.x);
        const double p_re = h1r * c.x - h1i * c.y, p_im = h1r * c.y + h1i * c.x;
        ur[r] = live ? u_re : 0.0;
        ui[r] = live ? u_im : 0.0;
        pw[r * 64 + lane] = (live && two) ? make_double2(p_re, p_im) : make_double2(0.0, 0.0);
        n_live += live;
        if constexpr (NV == 2) {
            const double x = nvs[row * R + r];
            nver[r] = x > 0.005 ? x : 0.005;
        }
    }
    __syncthreads();
    const double2 *ps = pw + sl * M;
    constexpr double INF = (double)INFINITY;
    double lo[LB > 0 ? LB : 1][2];            // minima over b by the low label bits q < LB of b (bit q = 1 << q)
    double hi[BPS - LB > 0 ? BPS - LB : 1][2];   // by the bits above, M > 16 only
    double best = INF;                        // min_b D(a, b), M > 16 only (else min(lo[0][0], lo[0][1]))
#pragma unroll
    for (int q = 0; q < LB; ++q) lo[q][0] = lo[q][1] = INF;
#pragma unroll
    for (int q = 0; q < BPS - LB; ++q) hi[q][0] = hi[q][1] = INF;
    for (int b0 = 0; b0 < M; b0 += UB) {
        double blk = INF;
#pragma unroll
        for (int k = 0; k < UB; ++k) {
            double D = 0.0;
#pragma unroll
            for (int r = 0; r < SM_MAX_R; ++r) {
                if (r >= R) break;
                const double2 p = ps[r * 64 + b0 + k];
                const double vr = ur[r] - p.x, vi = ui[r] - p.y;
                double d = vr * vr + vi * vi;
                if constexpr (NV == 2) d = d / nver[r];
                D = r ? D + d : d;
            }
#pragma unroll
            for (int q = 0; q < LB; ++q) lo[q][(k >> q) & 1] = sm_min(lo[q][(k >> q) & 1], D);
            if constexpr (M > UB) blk = sm_min(blk, D);
        }
        if constexpr (M > UB) {
            best = sm_min(best, blk);
#pragma unroll
            for (int q = 0; q < BPS - LB; ++q) {
                if ((b0 >> (LB + q)) & 1) hi[q][1] = sm_min(hi[q][1], blk);
                else hi[q][0] = sm_min(hi[q][0], blk);
            }
        }
    }
    if constexpr (M <= UB) best = sm_min(lo[0][0], lo[0][1]);
    // LLR i of the slot, i = stream * BPS + j, bit j MSB first: label bit q = BPS - 1 - j
    double diff = 0.0;
#pragma unroll
    for (int j = 0; j < BPS; ++j) {
        const int q = BPS - 1 - j;
        const bool one = (a >> q) & 1;
        const double a0 = sm_group_min<M>(one ? INF : best), a1 = sm_group_min<M>(one ? best : INF);
        const double s0 = q < LB ? lo[q < LB ? q : 0][0] : hi[q >= LB ? q - LB : 0][0];
        const double s1 = q < LB ? lo[q < LB ? q : 0][1] : hi[q >= LB ? q - LB : 0][1];
        const double b0m = sm_group_min<M>(s0), b1m = sm_group_min<M>(s1);
        if (a == j) diff = a0 - a1;
        if (a == BPS + j) diff = b0m - b1m;
    }
    const int n_out = two ? 2 * BPS : BPS;
    if (!in || a >= n_out) return;
    double l = diff;
    if constexpr (NV != 2) {
        const double x = NV == 1 ? nvs[row] : nv;
        l = diff / (x > 0.005 ? x : 0.005);
    }
    float o = 0.0f;
    if (n_live && l == l) o = sgn * (float)(l < -30.0 ? -30.0 : (l > 30.0 ? 30.0 : l));
    llr[row * stride + (long)2 * m * BPS + a] = o;
}

}  // namespace tdec
