// tdec_llrq.hip -- quantised channel LLRs (include/llrq.h): the de-puncture
// kernels that widen int8 / float16 rows on the fly, and the device quantiser.  All three are
// kernel templates, so the code object lists them after every earlier kernel (the manifest in
// tdec_api.hip names them last).
#pragma once

namespace tdec {

// Element kinds of a narrow LLR row (llrq.h: LLRQ_INT8, LLRQ_F16).
constexpr int Q_INT8 = 0, Q_F16 = 1;
template <int KIND> struct QElem { using type = int8_t; };
template <> struct QElem<Q_F16> { using type = _Float16; };

// int8: (float)q * step, one f32 multiply (-128 is -128 * step).  f16: (float)x, exact:
// infinities and NaN pass through, subnormal halves are kept (step is 1 and not applied).
template <int KIND>
__device__ __forceinline__ float q_widen(typename QElem<KIND>::type x, float step) {
    if constexpr (KIND == Q_INT8) return (float)x * step;
    else return (float)x;
}

// Trellis steps one lane covers.  The LLRs of steps k .. k + Q_STEPS - 1 of one codeword are one
// contiguous run of its row (at most 6 per step), so a lane's 1- or 2-byte loads walk up to 48
// consecutive bytes instead of striding the row once per step as k_depuncture's thread shape
// would make them; each load's offset is wave-uniform (src[] by scalar loads) and needs no
// alignment, so any stride and any row base take the same path.  The plane stores are
// k_depuncture's: per step, 64 lanes write 1 KiB of float4 and 512 B of float2.
constexpr int Q_STEPS = 8;
// per kind: the same 48 bytes per lane for both (8 int8 steps, 4 float16 steps), so a wave's runs cover as many
// cache lines either way (measured, DESIGN.md §17: float16 at 8 steps ran 24 % behind the float32 kernel)
template <int KIND> constexpr int q_steps() { return KIND == Q_F16 ? Q_STEPS / 2 : Q_STEPS; }

// k_depuncture on narrow rows: the same planes bit for bit as k_depuncture on the widened rows
// (punctured and missing components and lanes past B are 0.0f).  total = tiles * ceil(N / steps) * 64.
template <int KIND>
__global__ __launch_bounds__(BLOCK) void k_depuncture_q(int B, int N, const typename QElem<KIND>::type *__restrict__ llr,
                                                       float step, long stride, const int *__restrict__ src,
                                                       float *__restrict__ planes, long total) {
    const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= total) return;
    constexpr int STEPS = q_steps<KIND>();
    const int groups = (N + STEPS - 1) / STEPS;
    const int lane = (int)(t & (WAVE - 1));
    const long q = t >> 6;                  // (tile, group): wave-uniform
    const int k0 = __builtin_amdgcn_readfirstlane((int)(q % groups)) * STEPS;
    const long tile = __builtin_amdgcn_readfirstlane((int)(q / groups));
    const long cw = tile * WAVE + lane;
    const bool live = cw < B;
    const typename QElem<KIND>::type *row = llr + (live ? cw : 0) * stride;
    float v[STEPS][6];
    const int comp[6] = {0, 1, 2, 3, 6, 7};
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            v[s][c] = 0.0f;
            if (k0 + s < N) {
                const int j = src[(long)comp[c] * N + k0 + s];
                if (j >= 0 && live) v[s][c] = q_widen<KIND>(row[j], step);
            }
        }
    }
    float *base = planes + tile * tile_floats(N);
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        if (k0 + s < N) {
            const long e = (long)(k0 + s) * WAVE + lane;
            reinterpret_cast<float4 *>(base)[e] = make_float4(v[s][0], v[s][1], v[s][2], v[s][3]);
            reinterpret_cast<float2 *>(base + (long)N * WAVE * 4)[e] = make_float2(v[s][4], v[s][5]);
        }
    }
}

// k_depuncture_acc on narrow rows, its contract to the letter: plane slot c takes row row_of[c]
// (null: row c); a slot whose entry is outside [0, n_rows) and a lane past n_slots are neither
// read nor written; a transmitted component becomes plane + value, one f32 add; one the pattern
// does not transmit is stored back as loaded.  The thread shape is k_depuncture_q's.
template <int KIND>
__global__ __launch_bounds__(BLOCK) void k_depuncture_acc_q(int n_slots, int N,
                                                           const typename QElem<KIND>::type *__restrict__ llr, float step,
                                                           long stride, int n_rows, const int *__restrict__ row_of,
                                                           const int *__restrict__ src, float *planes, long total) {
    const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= total) return;
    constexpr int STEPS = q_steps<KIND>();
    const int groups = (N + STEPS - 1) / STEPS;
    const int lane = (int)(t & (WAVE - 1));
    const long q = t >> 6;
    const int k0 = __builtin_amdgcn_readfirstlane((int)(q % groups)) * STEPS;
    const long tile = __builtin_amdgcn_readfirstlane((int)(q / groups));
    const long slot = tile * WAVE + lane;
    if (slot >= n_slots) return;
    const long r = row_of ? (long)row_of[slot] : slot;
    if (r < 0 || r >= n_rows) return;
    const typename QElem<KIND>::type *row = llr + r * stride;
    float *base = planes + tile * tile_floats(N);
    const int comp[6] = {0, 1, 2, 3, 6, 7};
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        if (k0 + s < N) {
            const long e = (long)(k0 + s) * WAVE + lane;
            float4 *px = reinterpret_cast<float4 *>(base) + e;
            float2 *pz = reinterpret_cast<float2 *>(base + (long)N * WAVE * 4) + e;
            float4 x = *px;
            float2 z = *pz;
            float *v[6] = {&x.x, &x.y, &x.z, &x.w, &z.x, &z.y};
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const int j = src[(long)comp[c] * N + k0 + s];
                if (j >= 0) *v[c] = *v[c] + q_widen<KIND>(row[j], step);
            }
            *px = x;
            *pz = z;
        }
    }
}

// The quantiser (llrq.h): q = (int8) clamp(rintf((float)x * inv_step), -127, 127), ties to even;
// NaN -> 0, +-inf -> +-127, -0.0 -> 0.  *sat is set when |x * inv_step| > 127 (the infinities
// included, NaN not).
__device__ __forceinline__ int q_quantize(float x, float inv_step, int *sat) {
    const float p = x * inv_step;
    *sat = fabsf(p) > 127.0f;
    if (p != p) return 0;
    return (int)fminf(fmaxf(rintf(p), -127.0f), 127.0f);
}

constexpr int QZ_VEC = 16;   // int8 outputs per 16-byte store

// Flat, grid-stride.  The output's 16-byte aligned middle is written 16 bytes per thread (its
// 16 inputs by 16-byte loads where the input is aligned there too, one by one where it is not);
// the head before the first aligned output byte and the tail after the last whole vector go one
// element per thread: the same arithmetic, so an offset base changes no value.  saturated
// (nullable) receives one 64-bit vector atomic add per block that counted any.
template <bool F64>
__global__ __launch_bounds__(BLOCK) void k_llr_quantize(const void *__restrict__ in_, long n, float inv_step,
                                                       int8_t *__restrict__ out, unsigned long long *saturated) {
    using T = typename std::conditional<F64, double, float>::type;
    const T *in = static_cast<const T *>(in_);
    const long head = std::min<long>(n, (long)((QZ_VEC - ((uintptr_t)out & (QZ_VEC - 1))) & (QZ_VEC - 1)));
    const long n_vec = (n - head) / QZ_VEC, tail0 = head + n_vec * QZ_VEC;
    const long gsz = (long)gridDim.x * BLOCK, t0 = (long)blockIdx.x * BLOCK + threadIdx.x;
    const bool in_aligned = ((uintptr_t)(in + head) & 15) == 0;   // wave-uniform
    unsigned long long count = 0;   // 64 bits throughout: the counter is exact for every n
    for (long i = t0; i < n_vec; i += gsz) {
        const T *p = in + head + i * QZ_VEC;
        T x[QZ_VEC];
        if (in_aligned) {
            constexpr int PER = 16 / (int)sizeof(T);   // elements per 16-byte load
            using V = typename std::conditional<F64, double2, float4>::type;
#pragma unroll
            for (int a = 0; a < QZ_VEC / PER; ++a) {
                const V w = reinterpret_cast<const V *>(p)[a];
                x[a * PER] = w.x, x[a * PER + 1] = w.y;
                if constexpr (!F64) x[a * PER + 2] = w.z, x[a * PER + 3] = w.w;
            }
        } else {
#pragma unroll
            for (int a = 0; a < QZ_VEC; ++a) x[a] = p[a];
        }
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int a = 0; a < QZ_VEC; ++a) {
            int s;
            const int v = q_quantize((float)x[a], inv_step, &s);
            count += s;
            w[a / 4] |= (unsigned)(v & 255) << (8 * (a % 4));
        }
        *reinterpret_cast<uint4 *>(out + head + i * QZ_VEC) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // head and tail: fewer than 32 elements in all
    const long n_edge = head + (n - tail0);
    for (long i = t0; i < n_edge; i += gsz) {
        const long e = i < head ? i : tail0 + (i - head);
        int s;
        out[e] = (int8_t)q_quantize((float)in[e], inv_step, &s);
        count += s;
    }
    if (!saturated) return;   // kernel-uniform
    __shared__ unsigned long long part[BLOCK / WAVE];
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) count += __shfl_down(count, d, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int w = 0; w < BLOCK / WAVE; ++w) sum += part[w];
        if (sum) atomicAdd(saturated, sum);
    }
}

}  // namespace tdec
