// tdec_stbc.hip -- transmit diversity (include/stbc.h): the Alamouti 2 x R
// combiner.  The generator's side is the StbcArgs branch of tdec_workload.hip.
//
// k_stbc_combine: y [B][R][S2] complex64 through the gains h [B][R][2][nh] into what
// k_equalize and k_combine write, z [B][S] and nv_sym [B][S].  All in f64, no contraction,
// the branches in the order r = 0 .. R-1; the terms and the order of their additions are
// include/stbc.h's, the skip, first-live-term, erasure and NaN rules k_combine's.
// One thread per pair of slots, consecutive lanes on consecutive pairs of one row: every
// branch's loads are coalesced, a pair's R branches lie S2 apart.  Y16: a pair's y is one
// 16-byte load (S2 is even, so every branch row is 16-byte aligned when the base is; the
// host checks the base), else two 8-byte ones.  VEC: z and nv_sym written 16 bytes at a
// time (S even and both bases 16-byte aligned: the host checks), else 8 bytes at a time,
// and the pad slot's second output (odd S) not at all.  No LDS, no barrier.
#include <hip/hip_runtime.h>

namespace tdec {

struct StbcSum {
    double G, ar, ai, br, bi;   // sums of g_r, num0_r (a) and num1_r (b)
    bool live;
};
struct StbcOut {
    float2 z0, z1;
    double nv;
};

template <int NV>
__device__ __forceinline__ void stbc_add(StbcSum &m, float2 y0, float2 y1, float2 h0, float2 h1, double nv_br) {
    const double h0r = (double)h0.x, h0i = (double)h0.y, h1r = (double)h1.x, h1i = (double)h1.y;
    const double y0r = (double)y0.x, y0i = (double)y0.y, y1r = (double)y1.x, y1i = (double)y1.y;
    const double g = (h0r * h0r + h0i * h0i) + (h1r * h1r + h1i * h1i);
    if (g == 0.0 || !(fabs(g) < INFINITY)) return;   // a dead branch vouches for nothing
    double gg = g;
    double ar = (y0r * h0r + y0i * h0i) + (y1r * h1r + y1i * h1i);
    double ai = (y0i * h0r - y0r * h0i) + (y1r * h1i - y1i * h1r);
    double br = (y0r * h1r + y0i * h1i) - (y1r * h0r + y1i * h0i);
    double bi = (y0i * h1r - y0r * h1i) - (y1r * h0i - y1i * h0r);
    if constexpr (NV == 2) {
        gg = g / nv_br;
        ar = ar / nv_br;
        ai = ai / nv_br;
        br = br / nv_br;
        bi = bi / nv_br;
    }
    if (m.live) {
        m.G += gg;
        m.ar += ar;
        m.ai += ai;
        m.br += br;
        m.bi += bi;
    } else {
        m = StbcSum{gg, ar, ai, br, bi, true};
    }
}

template <int NV>
__device__ __forceinline__ StbcOut stbc_out(const StbcSum &m, double nv) {
    if (!m.live || m.G == 0.0 || fabs(m.G) == (double)INFINITY)
        return StbcOut{make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f), (double)INFINITY};
    return StbcOut{make_float2((float)(m.ar / m.G), (float)(m.ai / m.G)),
                   make_float2((float)(m.br / m.G), (float)(m.bi / m.G)), (NV == 2 ? 1.0 : nv) / m.G};
}

// n_pairs = B * S2 / 2; nvs: [B] (NV 1) or [B][R] (NV 2)
template <int NV, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_stbc_combine(const float2 *y, const float2 *h, long n_pairs, int R, int S,
                                                       int coh, int nh, bool y16, double nv, const double *nvs,
                                                       float2 *z, double *nv_sym) {
    const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_pairs) return;
    const int S2 = S + (S & 1), P = S2 >> 1;
    const long row = t / P;
    const int s = 2 * (int)(t - row * P);            // the pair's even slot
    const float2 *yb = y + row * R * S2 + s, *hb = h + row * R * 2 * nh + s / coh;
    const double nv_c = NV == 1 ? nvs[row] : nv;
    StbcSum m{};
    for (int r = 0; r < R; ++r) {
        const double nv_br = NV == 2 ? nvs[row * R + r] : 0.0;
        const float2 *yr = yb + (long)r * S2;
        float2 y0, y1;
        if (y16) {
            const float4 yy = *reinterpret_cast<const float4 *>(yr);
            y0 = make_float2(yy.x, yy.y);
            y1 = make_float2(yy.z, yy.w);
        } else {
            y0 = yr[0];
            y1 = yr[1];
        }
        stbc_add<NV>(m, y0, y1, hb[(2 * r) * nh], hb[(2 * r + 1) * nh], nv_br);
    }
    const StbcOut o = stbc_out<NV>(m, nv_c);
    const long i = row * S + s;
    if constexpr (VEC) {                             // S even: i is even, and s + 1 < S
        *reinterpret_cast<float4 *>(z + i) = make_float4(o.z0.x, o.z0.y, o.z1.x, o.z1.y);
        *reinterpret_cast<double2 *>(nv_sym + i) = make_double2(o.nv, o.nv);
    } else {
        z[i] = o.z0;
        nv_sym[i] = o.nv;
        if (s + 1 < S) {
            z[i + 1] = o.z1;
            nv_sym[i + 1] = o.nv;
        }
    }
}

}  // namespace tdec
