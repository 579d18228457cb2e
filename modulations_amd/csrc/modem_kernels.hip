// modem_kernels.hip -- gfx950 kernels of the modem front-end (SURVEY.md §8(f)
// row 4): mappers, hard demodulators, polyphase FIR, IQ sample conversion.
//
// All of these are byte-moving elementwise passes (HBM-bound): one thread per
// output element, grid-stride, tables staged once per block in LDS, the FIR's
// input window staged in LDS so every input sample is fetched from HBM once
// per block.  Arithmetic restates the reference's numpy expressions in the
// precision numpy uses for them (npmath.hip); the build keeps IEEE denormals
// and no FMA contraction (-ffp-contract=off), explicit fma() only where
// numpy's own loop fuses (|z|) or where the reference's sum order is not
// defined (the FIR: BLAS / scipy order, compared within a tolerance).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "npmath.hip"

namespace mdm {

constexpr int BLOCK = 256;
constexpr int MAP_MAX = 256;    // points of a mapper table (f32; 128 for f64)
constexpr int TAPS_MAX = 256;   // FIR taps
constexpr int ARG_MAX = 64;     // points of an argmin table

__device__ __forceinline__ long gtid() { return (long)blockIdx.x * BLOCK + threadIdx.x; }
__device__ __forceinline__ long gstride() { return (long)gridDim.x * BLOCK; }

// ---- mapper: bits (MSB-first labels, zero padded) -> table[label] ---------------------
struct MapTable {
    union {
        float f[2 * MAP_MAX];
        double d[MAP_MAX];   // MAP_MAX/2 complex128 points
    };
};

template <typename T> struct C2;
template <> struct C2<float> { typedef float2 t; };
template <> struct C2<double> { typedef double2 t; };

// One block-iteration maps MAP_SPB symbols: their label bytes (MAP_SPB * bps
// <= 8 KiB) are staged in LDS with 16-B loads, then every thread reads its
// symbols' bits from LDS and the stores run coalesced (consecutive threads,
// consecutive symbols).
constexpr int MAP_SPB = 1024;

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_map(const uint8_t *__restrict__ bits, long n_bits, int bps, long n_sym,
                                               MapTable tab, typename C2<T>::t *__restrict__ out) {
    typedef typename C2<T>::t V;
    __shared__ V t[MAP_MAX];
    __shared__ uint4 lb[MAP_SPB * 8 / 16];
    const T *src = sizeof(T) == 4 ? (const T *)tab.f : (const T *)tab.d;
    for (int i = threadIdx.x; i < (1 << bps); i += BLOCK) {
        V v;
        v.x = src[2 * i];
        v.y = src[2 * i + 1];
        t[i] = v;
    }
    const uint8_t *lbytes = reinterpret_cast<const uint8_t *>(lb);
    for (long s0 = (long)blockIdx.x * MAP_SPB; s0 < n_sym; s0 += (long)gridDim.x * MAP_SPB) {
        const long b0 = s0 * bps;                       // first label byte of the block
        const long nb = min((long)MAP_SPB * bps, n_bits - b0);
        __syncthreads();
        if (((uintptr_t)(bits + b0) & 15) == 0 && nb == (long)MAP_SPB * bps) {
            const uint4 *g = reinterpret_cast<const uint4 *>(bits + b0);
            for (int i = threadIdx.x; i < MAP_SPB * bps / 16; i += BLOCK) lb[i] = g[i];
        } else {
            uint8_t *l = reinterpret_cast<uint8_t *>(lb);
            for (int i = threadIdx.x; i < MAP_SPB * bps; i += BLOCK) l[i] = i < nb ? bits[b0 + i] : 0;
        }
        __syncthreads();
        const int ns = (int)min((long)MAP_SPB, n_sym - s0);
        for (int j = threadIdx.x; j < ns; j += BLOCK) {
            int lab = 0;
            for (int q = 0; q < bps; ++q) lab = (lab << 1) | (lbytes[j * bps + q] & 1);
            out[s0 + j] = t[lab];
        }
    }
}

// ---- hard demodulators -------------------------------------------------------------------
struct DemodArgs {
    int kind, bps, nan_raises, levels, vec;   // vec: the output rows are aligned for one store per symbol
    double scale;
    int32_t labels[256];
    double cons[2 * ARG_MAX];
};

// round(angle / (pi/4)) of the 8PSK demods in the symbols' precision:
// np.angle -> arctan2; `if phase < 0: phase += 2*np.pi` (a Python float added
// to a numpy scalar of the symbols' dtype stays in that dtype); / (np.pi/4);
// np.round = round half to even.
template <typename T> __device__ __forceinline__ T psk8_sector(T re, T im) {
    T ph = atan2(im, re);
    if (ph < (T)0) ph = ph + (T)6.283185307179586;
    return rint(ph / (T)0.7853981633974483);
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_demod(const typename C2<T>::t *__restrict__ syms, long n_sym, DemodArgs a,
                                                 uint8_t *__restrict__ bits, uint32_t *__restrict__ nan_count) {
    __shared__ int lab[256];
    __shared__ double cons[2 * ARG_MAX];
    for (int i = threadIdx.x; i < 256; i += BLOCK) lab[i] = a.labels[i];
    for (int i = threadIdx.x; i < 2 * ARG_MAX; i += BLOCK) cons[i] = a.cons[i];
    __syncthreads();
    uint32_t nans = 0;
    for (long s = gtid(); s < n_sym; s += gstride()) {
        const T re = syms[s].x, im = syms[s].y;
        uint8_t ob[8];
        uint8_t *o = ob;
        if (a.kind == 0) {                      // MDM_DEMOD_GT0
            o[0] = re > (T)0;
        } else if (a.kind == 1) {               // MDM_DEMOD_QPSK
            o[0] = re < (T)0;
            o[1] = im < (T)0;
        } else if (a.kind == 2) {               // MDM_DEMOD_PSK8
            const T r = psk8_sector<T>(re, im);
            int idx = 0;
            if (r != r) nans += a.nan_raises;   // int(NaN) raises; astype(int) -> INT64_MIN, % 8 = 0
            else idx = ((int)r) & 7;            // r in [0, 8]
            const int l = lab[idx];
            o[0] = (l >> 2) & 1;
            o[1] = (l >> 1) & 1;
            o[2] = l & 1;
        } else if (a.kind == 3) {               // MDM_DEMOD_QAM_AXIS (f64, np.float64 scale)
            const int K = a.bps / 2, L = a.levels;
#pragma unroll
            for (int ax = 0; ax < 2; ++ax) {
                const double x = (double)(ax ? im : re) * a.scale;
                double q = rint((x + (double)(L - 1)) / 2.0);
                int idx = 0;
                if (q != q) nans += 1;          // int(np.clip(np.round(NaN))) raises
                else {
                    q = q < 0.0 ? 0.0 : (q > (double)(L - 1) ? (double)(L - 1) : q);
                    idx = (int)q;
                }
                const int l = lab[idx];
                for (int b = 0; b < K; ++b) o[ax * K + b] = (l >> (K - 1 - b)) & 1;
            }
        } else {                                // MDM_DEMOD_ARGMIN: first index of the minimum, NaN wins
            const int M = 1 << a.bps;
            const double sr = (double)re, si = (double)im;
            int idx = 0;
            double best = npm::cabs_np<double>(sr - cons[0], si - cons[1]);
            for (int m = 1; m < M; ++m) {
                if (best != best) break;
                const double d = npm::cabs_np<double>(sr - cons[2 * m], si - cons[2 * m + 1]);
                if (d < best || d != d) {
                    best = d;
                    idx = m;
                }
            }
            for (int b = 0; b < a.bps; ++b) o[b] = (idx >> (a.bps - 1 - b)) & 1;
        }
        // one store per symbol where the width allows (the rows stay coalesced)
        uint8_t *dst = bits + s * a.bps;
        if (a.vec && a.bps == 8) {
            *reinterpret_cast<uint2 *>(dst) = make_uint2(ob[0] | ob[1] << 8 | ob[2] << 16 | (unsigned)ob[3] << 24,
                                                         ob[4] | ob[5] << 8 | ob[6] << 16 | (unsigned)ob[7] << 24);
        } else if (a.vec && a.bps == 4) {
            *reinterpret_cast<unsigned *>(dst) = ob[0] | ob[1] << 8 | ob[2] << 16 | (unsigned)ob[3] << 24;
        } else if (a.vec && a.bps == 2) {
            *reinterpret_cast<unsigned short *>(dst) = (unsigned short)(ob[0] | ob[1] << 8);
        } else {
            for (int b = 0; b < a.bps; ++b) dst[b] = ob[b];
        }
    }
    if (nan_count && nans) atomicAdd(nan_count, nans);
}

// ---- polyphase up-sample / FIR / down-sample ------------------------------------------
//   out[i] = sum_k h[k] * xu[i*down + off - k],  xu[j] = x[j/up] (j % up == 0, in range) else 0
// One block = FIR_OPB consecutive outputs; the input samples they touch are
// staged once in LDS (as f64) when they fit, else read through L1/L2.
struct FirArgs {
    int n_taps, up, down, per_thread;
    long off, n_out, n_x;
    double h[TAPS_MAX];
};
constexpr int FIR_LDS = 3840;   // staged input samples (60 KiB of double2)

__device__ __forceinline__ int fdiv_floor(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// Index arithmetic is 32-bit (the host bounds n_out*down + off and n_x*up);
// per output one division by `up` finds the first tap and its input sample,
// then the tap loop steps k += up, m -= 1.
template <typename T, bool STAGE>
__global__ __launch_bounds__(BLOCK) void k_fir(const typename C2<T>::t *__restrict__ x, FirArgs a,
                                               double2 *__restrict__ out) {
    __shared__ double h[TAPS_MAX];
    __shared__ double2 xs[STAGE ? FIR_LDS : 1];
    for (int i = threadIdx.x; i < a.n_taps; i += BLOCK) h[i] = a.h[i];
    const int up = a.up, down = a.down, L = a.n_taps, nx = (int)a.n_x, off = (int)a.off;
    const int opb = BLOCK * a.per_thread;
    const int i0 = (int)blockIdx.x * opb;
    // input samples of this block's outputs: m in [m_lo, m_hi]
    int m_lo = -fdiv_floor(-(i0 * down + off - (L - 1)), up);   // ceil(j_lo / up)
    int m_hi = fdiv_floor((i0 + opb - 1) * down + off, up);
    m_lo = m_lo < 0 ? 0 : m_lo;
    m_hi = m_hi > nx - 1 ? nx - 1 : m_hi;
    if (STAGE) {
        for (int m = m_lo + threadIdx.x; m <= m_hi; m += BLOCK) {
            const typename C2<T>::t v = x[m];
            xs[m - m_lo] = make_double2((double)v.x, (double)v.y);
        }
    }
    __syncthreads();
    for (int r = 0; r < a.per_thread; ++r) {
        const int i = i0 + r * BLOCK + threadIdx.x;
        if (i >= (int)a.n_out) break;
        const int j0 = i * down + off;
        // first tap k >= max(0, j0 - (nx-1)*up) with k == j0 (mod up); its sample m = (j0 - k) / up
        const int mq = j0 / up, k_first = j0 - mq * up;           // largest m = mq (k = j0 mod up)
        int m = mq < nx - 1 ? mq : nx - 1;
        int k = j0 - m * up;
        if (k < k_first) k = k_first;
        const int kmax = j0 < L - 1 ? j0 : L - 1;
        double re = 0.0, im = 0.0;
        for (; k <= kmax; k += up, --m) {
            double xr, xi;
            if (STAGE) {
                const double2 v = xs[m - m_lo];
                xr = v.x;
                xi = v.y;
            } else {
                const typename C2<T>::t v = x[m];
                xr = (double)v.x;
                xi = (double)v.y;
            }
            re = fma(h[k], xr, re);
            im = fma(h[k], xi, im);
        }
        out[i] = make_double2(re, im);
    }
}

// Up-sampling form (down == 1), polyphase: thread = one input period m, i.e.
// the UP outputs j = m*UP + p, p < UP, which all read x[m], x[m-1], ... : each
// input sample is read from LDS once per period (not once per output) and the
// taps h[p + r*UP] are wave-uniform (LDS broadcast).  Per output the terms are
// summed in ascending k, exactly as k_fir does, so both forms agree bit for bit.
template <typename T, int UP>
__global__ __launch_bounds__(BLOCK) void k_fir_up(const typename C2<T>::t *__restrict__ x, FirArgs a,
                                                  double2 *__restrict__ out) {
    __shared__ double h[TAPS_MAX];
    __shared__ double2 xs[BLOCK + TAPS_MAX];
    for (int i = threadIdx.x; i < a.n_taps; i += BLOCK) h[i] = a.h[i];
    const int L = a.n_taps, nx = (int)a.n_x, off = (int)a.off, n_out = (int)a.n_out;
    const int R = (L + UP - 1) / UP;                 // input samples per period
    const int nper = (n_out - 1 + off) / UP + 1;     // periods holding outputs
    for (int m0 = (int)blockIdx.x * BLOCK; m0 < nper; m0 += (int)gridDim.x * BLOCK) {
        __syncthreads();
        const int lo = m0 - (R - 1);                 // xs[q] = x[lo + q], zero outside [0, nx)
        for (int q = threadIdx.x; q < BLOCK + R - 1; q += BLOCK) {
            const int mm = lo + q;
            if (mm >= 0 && mm < nx) {
                const typename C2<T>::t v = x[mm];
                xs[q] = make_double2((double)v.x, (double)v.y);
            } else {
                xs[q] = make_double2(0.0, 0.0);
            }
        }
        __syncthreads();
        const int m = m0 + threadIdx.x;
        if (m >= nper) continue;
        double re[UP], im[UP];
#pragma unroll
        for (int p = 0; p < UP; ++p) re[p] = im[p] = 0.0;
        for (int r = 0; r < R; ++r) {
            const int mm = m - r;
            if (mm < 0 || mm >= nx) continue;            // the term is absent (not a zero term)
            const double2 v = xs[threadIdx.x + R - 1 - r];
#pragma unroll
            for (int p = 0; p < UP; ++p) {
                const int k = p + r * UP;
                if (k < L) {
                    const double hk = a.h[k];   // wave-uniform: scalar load from the kernel arguments
                    re[p] = fma(hk, v.x, re[p]);
                    im[p] = fma(hk, v.y, im[p]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < UP; ++p) {
            const int i = m * UP + p - off;
            if (i >= 0 && i < n_out) out[i] = make_double2(re[p], im[p]);
        }
    }
}

// Decimating form (up == 1): thread = one output; the staged window is stored
// phase-major (sample q at [q % DOWN][q / DOWN]) so the wave's reads of
// x[i*DOWN + off - k] at one tap hit consecutive LDS words (no bank conflicts).
template <typename T, int DOWN>
__global__ __launch_bounds__(BLOCK) void k_fir_dec(const typename C2<T>::t *__restrict__ x, FirArgs a,
                                                   double2 *__restrict__ out) {
    constexpr int PL = (BLOCK * DOWN + TAPS_MAX + DOWN - 1) / DOWN + 1;   // samples per phase plane
    __shared__ double h[TAPS_MAX];
    __shared__ double2 xs[DOWN * PL];
    for (int i = threadIdx.x; i < a.n_taps; i += BLOCK) h[i] = a.h[i];
    const int L = a.n_taps, nx = (int)a.n_x, off = (int)a.off, n_out = (int)a.n_out;
    for (int i0 = (int)blockIdx.x * BLOCK; i0 < n_out; i0 += (int)gridDim.x * BLOCK) {
        __syncthreads();
        const int lo = i0 * DOWN + off - (L - 1);     // first sample the block reads
        const int span = (BLOCK - 1) * DOWN + L;
        for (int q = threadIdx.x; q < span; q += BLOCK) {
            const int mm = lo + q;
            double2 v = make_double2(0.0, 0.0);
            if (mm >= 0 && mm < nx) {
                const typename C2<T>::t w = x[mm];
                v = make_double2((double)w.x, (double)w.y);
            }
            xs[(q % DOWN) * PL + q / DOWN] = v;
        }
        __syncthreads();
        const int i = i0 + threadIdx.x;
        if (i >= n_out) continue;
        const int j0 = i * DOWN + off;
        double re = 0.0, im = 0.0;
        // k in ascending order over the taps whose sample lies in [0, nx)
        const int kmin = j0 - (nx - 1) > 0 ? j0 - (nx - 1) : 0;
        const int kmax = j0 < L - 1 ? j0 : L - 1;
        for (int k = kmin; k <= kmax; ++k) {
            const int q = j0 - k - lo;                    // = threadIdx.x*DOWN + (L-1-k)
            const double2 v = xs[(q % DOWN) * PL + q / DOWN];
            re = fma(h[k], v.x, re);
            im = fma(h[k], v.y, im);
        }
        out[i] = make_double2(re, im);
    }
}

// ---- IQ sample conversion ------------------------------------------------------------------
// max|sig| (np.max(np.abs(sig)), NaN propagating) as the largest bit pattern:
// abs values are >= +0, so their IEEE bits order like unsigned integers and a
// NaN outranks +inf.
// numpy's |z| (a division and a square root) is evaluated only for samples
// that can still be the maximum: a sample whose re^2 + im^2 (f64, < 1e-15
// relative error) is below (1 - margin) x that of the largest sample seen by
// this thread has a smaller numpy |z| than that sample (numpy's |z| is within
// a few ulp of the true modulus: margin 1e-9 for complex128, 1e-5 for
// complex64), so skipping it cannot change the maximum.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_absmax(const typename C2<T>::t *__restrict__ sig, long n,
                                                  unsigned long long *__restrict__ mx) {
    unsigned long long m = 0;
    double thr = -1.0;   // (1 - 1e-9) * largest re^2 + im^2 seen so far
    for (long i = gtid(); i < n; i += gstride()) {
        const double re = (double)sig[i].x, im = (double)sig[i].y;
        const double q = fma(re, re, im * im);
        if (q < thr) continue;                          // NaN q fails the test and is evaluated
        const T a = npm::cabs_np<T>(sig[i].x, sig[i].y);
        unsigned long long b;
        if (sizeof(T) == 8) b = (unsigned long long)__double_as_longlong((double)a);
        else b = (unsigned long long)(unsigned)__float_as_uint((float)a);
        m = b > m ? b : m;
        const double t = q * (sizeof(T) == 8 ? 1.0 - 1e-9 : 1.0 - 1e-5);
        thr = t > thr ? t : thr;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(m, o, 64);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(mx, m);
}

template <typename T> __device__ __forceinline__ int8_t to_i8(T v) {
    v = v * (T)127;                                           // np.real(sig) * 127
    if (v != v) return 0;                                     // astype(int8) of NaN (x86 numpy)
    v = v < (T)-127 ? (T)-127 : (v > (T)127 ? (T)127 : v);    // np.clip
    return (int8_t)(int)v;                                    // C cast: truncation toward zero
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_quantize(const typename C2<T>::t *__restrict__ sig, long n,
                                                    const unsigned long long *__restrict__ mx,
                                                    char2 *__restrict__ iq) {
    T amax;
    if (sizeof(T) == 8) amax = (T)__longlong_as_double((long long)*mx);
    else amax = (T)__uint_as_float((unsigned)*mx);
    const T d = amax + (T)1e-10;   // np.max(...) + 1e-10 in the signal's precision
    for (long i = gtid(); i < n; i += gstride()) {
        T qr, qi, pr, pi;
        npm::cdiv_np<T>(sig[i].x, sig[i].y, d, (T)0, qr, qi);       // sig / d (complex division)
        npm::cmul_np<T>(qr, qi, (T)0.95, (T)0, pr, pi);              // * 0.95 (complex product)
        iq[i] = make_char2(to_i8<T>(pr), to_i8<T>(pi));
    }
}

// (raw.astype(np.float32) - 127.5) / 127.5, I from even bytes, Q from odd.
// 8 samples (16 B in, 64 B out) per thread and step when both buffers are
// 16-B aligned; the remaining samples one by one.
__device__ __forceinline__ float deq(unsigned b) { return ((float)b - 127.5f) / 127.5f; }

__global__ __launch_bounds__(BLOCK) void k_dequantize(const uint8_t *__restrict__ raw, long n, float2 *__restrict__ sig,
                                                      int vec) {
    const long n8 = vec ? n / 8 : 0;   // vec: both buffers 16-B aligned
    const uint4 *r16 = reinterpret_cast<const uint4 *>(raw);
    float4 *o16 = reinterpret_cast<float4 *>(sig);
    for (long i = gtid(); i < n8; i += gstride()) {
        const uint4 r = r16[i];
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o16[4 * i + q] = make_float4(deq(w[q] & 255), deq((w[q] >> 8) & 255), deq((w[q] >> 16) & 255),
                                         deq(w[q] >> 24));
    }
    for (long i = 8 * n8 + gtid(); i < n; i += gstride())
        sig[i] = make_float2(deq(raw[2 * i]), deq(raw[2 * i + 1]));
}

// ======================================================================================
// Receive chain (sdr_modem.py:282-325, 528-579): mixer, burst detector, sync correlator,
// carrier loops.  DESIGN.md "Receive chain".
// ======================================================================================

// non-negative f64 (or NaN) -> bits that order like the values, a NaN above +inf
__device__ __forceinline__ unsigned long long ord_bits(double v) {
    return (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffULL;
}

// ---- _correct_freq (:282-285): out[i] = (sig[i] - dc) * exp(j * w * ((i0 + i) / fs)) -----------
// np.exp of (+-0 + j theta) is (cos theta, sin theta); the product is numpy's complex128 one.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mix(const typename C2<T>::t *__restrict__ sig, long n, long i0, int has_dc,
                                               T dcr, T dci, double w, double fs, double2 *__restrict__ out) {
    for (long i = gtid(); i < n; i += gstride()) {
        T re = sig[i].x, im = sig[i].y;
        if (has_dc) {
            re = re - dcr;
            im = im - dci;
        }
        const double th = w * ((double)(i0 + i) / fs);
        double sn, cs, pr, pi;
        sincos(th, &sn, &cs);
        npm::cmul_np<double>((double)re, (double)im, cs, sn, pr, pi);
        out[i] = make_double2(pr, pi);
    }
}

// ---- power detection (:528-546) -------------------------------------------------------------
// One workgroup = BF_TILE consecutive outputs of np.convolve(power, ones(win)/win, 'same'):
//   smooth[i] = (1/win) * sum_{m = i - win/2}^{i - win/2 + win - 1} power[m]   (0 outside [0, n)).
// The tile's window (BF_TILE + win - 1 <= 2047 samples) is summed into an exclusive prefix
// array in LDS (8 consecutive samples per thread, wave scan, cross-wave carry); an output is
// the difference of two prefix values.  Rounding: a prefix value carries <= ~20 eps of the
// window's sum (<= 2047 max(power)), so after the 1/win an output is within ~50 eps
// max(power) of the exact mean -- the reference's own dot product is no closer.
constexpr int BF_TILE = 1024;
constexpr int BF_WIN_MAX = 1024;
constexpr int BF_PER = (BF_TILE + BF_WIN_MAX) / BLOCK;   // window samples per thread (8)

template <typename T>
__device__ __forceinline__ double bf_power(const typename C2<T>::t *__restrict__ sig, long m, long n, T dcr, T dci) {
    if (m < 0 || m >= n) return 0.0;
    const typename C2<T>::t v = sig[m];
    const T a = npm::cabs_np<T>(v.x - dcr, v.y - dci);   // np.abs(rx) in the signal's precision
    return (double)(a * a);                              // ** 2, then convolve's float64
}

// fills P[q] = sum of the window's first q samples, q <= BF_TILE + win - 1 (window sample q is
// power[i0 - win/2 + q]); ends with a barrier
template <typename T>
__device__ __forceinline__ void bf_prefix(const typename C2<T>::t *__restrict__ sig, long n, T dcr, T dci, int win,
                                          long i0, double *P, double *wsum) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long m0 = i0 - win / 2 + (long)t * BF_PER;
    const int span = BF_TILE + win - 1;
    double e[BF_PER], s = 0.0;
#pragma unroll
    for (int j = 0; j < BF_PER; ++j) {
        e[j] = s;
        s += t * BF_PER + j < span ? bf_power<T>(sig, m0 + j, n, dcr, dci) : 0.0;
    }
    double inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    double base = 0.0;
    for (int k = 0; k < wave; ++k) base += wsum[k];
    const double excl = base + (inc - s);
#pragma unroll
    for (int j = 0; j < BF_PER; ++j) P[t * BF_PER + j] = excl + e[j];
    __syncthreads();
}

// launch 1: smoothed power (stored when asked for) and its maximum (bit pattern, atomicMax)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_bf_smooth(const typename C2<T>::t *__restrict__ sig, long n, T dcr, T dci,
                                                     int win, double *__restrict__ smooth,
                                                     unsigned long long *__restrict__ mx) {
    __shared__ double P[BF_TILE + BF_WIN_MAX];
    __shared__ double wsum[BLOCK / 64];
    const long i0 = (long)blockIdx.x * BF_TILE;
    bf_prefix<T>(sig, n, dcr, dci, win, i0, P, wsum);
    const double inv = 1.0 / (double)win;
    unsigned long long m = 0;
    for (int j = threadIdx.x; j < BF_TILE; j += BLOCK) {
        if (i0 + j >= n) break;
        const double v = (P[j + win] - P[j]) * inv;
        if (smooth) smooth[i0 + j] = v;
        const unsigned long long b = ord_bits(v);
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(m, o, 64);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(mx, m);
}

// launch 2: flags = smooth > 0.3 * max, and per tile the first zero flag, the last zero flag
// and the first start p+1 behind a zero at p whose next zero in the tile is >= half away
// (int4: first, last, start, unused; tile-local, -1 = none).  Samples past n count as set.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_bf_flags(const typename C2<T>::t *__restrict__ sig, long n, T dcr, T dci,
                                                    int win, long half, const unsigned long long *__restrict__ mx,
                                                    int4 *__restrict__ tiles) {
    __shared__ double P[BF_TILE + BF_WIN_MAX];
    __shared__ double wsum[BLOCK / 64];
    __shared__ int wlast[BLOCK / 64], rfirst[BLOCK / 64], rlast[BLOCK / 64], rstart[BLOCK / 64];
    const long i0 = (long)blockIdx.x * BF_TILE;
    bf_prefix<T>(sig, n, dcr, dci, win, i0, P, wsum);
    const double inv = 1.0 / (double)win;
    const double thr = __longlong_as_double((long long)*mx) * 0.3;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    constexpr int PER = BF_TILE / BLOCK;   // 4 consecutive positions per thread
    bool z[PER];
    int first = BF_TILE, last = -1;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int j = t * PER + r;
        const double v = (P[j + win] - P[j]) * inv;
        z[r] = i0 + j < n && !(v > thr);
        if (z[r]) {
            first = first < j ? first : j;
            last = j;
        }
    }
    // inclusive prefix maximum of `last` over the threads of the block
    int inc = last;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc = v > inc ? v : inc;
    }
    if (lane == 63) wlast[wave] = inc;
    int prev = __shfl_up(inc, 1, 64);   // last zero before this thread's positions
    if (lane == 0) prev = -1;
    __syncthreads();
    for (int k = 0; k < wave; ++k) prev = wlast[k] > prev ? wlast[k] : prev;
    int start = BF_TILE + 1;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int j = t * PER + r;
        if (z[r]) {
            if (prev >= 0 && (long)(j - prev - 1) >= half) start = start < prev + 1 ? start : prev + 1;
            prev = j;
        }
    }
    int lmax = last;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(first, o, 64), b = __shfl_xor(lmax, o, 64), c = __shfl_xor(start, o, 64);
        first = a < first ? a : first;
        lmax = b > lmax ? b : lmax;
        start = c < start ? c : start;
    }
    if (lane == 0) {
        rfirst[wave] = first;
        rlast[wave] = lmax;
        rstart[wave] = start;
    }
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < BLOCK / 64; ++k) {
            first = rfirst[k] < first ? rfirst[k] : first;
            lmax = rlast[k] > lmax ? rlast[k] : lmax;
            start = rstart[k] < start ? rstart[k] : start;
        }
        tiles[blockIdx.x] = make_int4(first < BF_TILE ? first : -1, lmax, start <= BF_TILE ? start : -1, 0);
    }
}

// launch 3 (one workgroup): the first i < n - preamble_len whose next `half` flags are all
// set.  Such an i is 0 or directly follows a zero flag, so it is the first p + 1 (p a zero
// flag, or -1) whose following zero is >= half away: a prefix maximum over the tiles' last
// zeros gives every tile the zero before it.
__global__ __launch_bounds__(BLOCK) void k_bf_scan(const int4 *__restrict__ tiles, long n_tiles, long n, long pre,
                                                   long half, long long *__restrict__ res) {
    __shared__ long long sc[BLOCK];
    __shared__ long long best[BLOCK];
    const int t = threadIdx.x;
    long long carry = -1, found = -1;
    for (long c0 = 0; c0 < n_tiles; c0 += BLOCK) {
        const long g = c0 + t;
        int4 s = make_int4(-1, -1, -1, 0);
        if (g < n_tiles) s = tiles[g];
        const long long base = (long long)g * BF_TILE;
        sc[t] = s.y >= 0 ? base + s.y : -1;
        __syncthreads();
        for (int o = 1; o < BLOCK; o <<= 1) {
            const long long v = t >= o ? sc[t - o] : -1;
            __syncthreads();
            sc[t] = v > sc[t] ? v : sc[t];
            __syncthreads();
        }
        long long prev = t ? sc[t - 1] : -1;
        prev = carry > prev ? carry : prev;
        long long cand = 0x7fffffffffffffffLL;
        if (s.x >= 0) {
            if (base + s.x - prev - 1 >= half) cand = prev + 1;
            else if (s.z >= 0) cand = base + s.z;
        }
        best[t] = cand;
        __syncthreads();
        for (int o = BLOCK / 2; o > 0; o >>= 1) {
            if (t < o) best[t] = best[t + o] < best[t] ? best[t + o] : best[t];
            __syncthreads();
        }
        const long long b = best[0], last = sc[BLOCK - 1];
        __syncthreads();
        if (b != 0x7fffffffffffffffLL) {
            found = b;
            break;
        }
        carry = last > carry ? last : carry;
    }
    if (found < 0) found = carry + 1;   // the run behind the last zero reaches the end
    if (t == 0) res[0] = found < n - pre ? found : -1;
}

// ---- sync search (:568-579): corr[i] = | sum_k region[i + k] * conj(w[k]) | and its argmax ----
// One workgroup = XC_OPB = 1024 consecutive outputs, XC_T = 4 per thread.  The taps (<= 1024,
// 16 KiB) and the window region[i0 .. i0 + 1024 + n_w - 1) (32 KiB) are staged once in LDS;
// the window is stored phase-major (sample q at plane q % 4, slot q / 4), so the wave's read
// of sample 4 t + c hits consecutive 16-B slots: a conflict-free ds_read_b128.  Per step of
// four taps a thread reads 4 new samples and 4 taps (wave-uniform, broadcast) for 16 complex
// MACs = 64 f64 FMAs: the loop is FMA-bound (the LDS is busy about half of the time).
// Per output the terms are added in ascending k with fma, real part rr*wr then ri*wi.
constexpr int XC_T = 4;
constexpr int XC_OPB = BLOCK * XC_T;
constexpr int XC_NW = 1024;
constexpr int XC_PL = (XC_OPB + XC_NW) / 4 + 1;   // slots per plane

struct XcBest {
    unsigned long long v;   // ord_bits of the value
    long long i;            // -1: none
};
__device__ __forceinline__ XcBest xc_better(XcBest a, XcBest b) {   // the larger value, the lower index on ties
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    if (a.v != b.v) return a.v > b.v ? a : b;
    return a.i < b.i ? a : b;
}
__device__ __forceinline__ XcBest xc_block_best(XcBest m, XcBest *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        XcBest q;
        q.v = __shfl_xor(m.v, o, 64);
        q.i = __shfl_xor(m.i, o, 64);
        m = xc_better(m, q);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    for (int k = 0; k < BLOCK / 64; ++k) m = k ? xc_better(m, sh[k]) : sh[0];
    return m;
}

__global__ __launch_bounds__(BLOCK) void k_xcorr(const double2 *__restrict__ region, long n_region,
                                                 const double2 *__restrict__ w, int n_w, long n_out,
                                                 double *__restrict__ corr, XcBest *__restrict__ part) {
    __shared__ double2 ws[XC_NW];
    __shared__ double2 xs[4 * XC_PL];
    __shared__ XcBest sh[BLOCK / 64];
    const int t = threadIdx.x;
    const long i0 = (long)blockIdx.x * XC_OPB;
    for (int i = t; i < XC_NW; i += BLOCK) ws[i] = i < n_w ? w[i] : make_double2(0.0, 0.0);
    for (int q = t; q < 4 * XC_PL; q += BLOCK) {
        const long m = i0 + q;
        xs[(q & 3) * XC_PL + (q >> 2)] = m < n_region ? region[m] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    double ar[XC_T], ai[XC_T];
#pragma unroll
    for (int o = 0; o < XC_T; ++o) ar[o] = ai[o] = 0.0;
    double2 a[7];   // samples 4 t + kk + 0..6
    a[0] = xs[0 * XC_PL + t];
    a[1] = xs[1 * XC_PL + t];
    a[2] = xs[2 * XC_PL + t];
    const int n_w4 = n_w & ~3;
    for (int kk = 0; kk < n_w4; kk += 4) {
        const int s = t + (kk >> 2);
        a[3] = xs[3 * XC_PL + s];
        a[4] = xs[0 * XC_PL + s + 1];
        a[5] = xs[1 * XC_PL + s + 1];
        a[6] = xs[2 * XC_PL + s + 1];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double2 c = ws[kk + u];
#pragma unroll
            for (int o = 0; o < XC_T; ++o) {
                const double2 x = a[o + u];
                ar[o] = fma(x.x, c.x, ar[o]);
                ar[o] = fma(x.y, c.y, ar[o]);
                ai[o] = fma(x.y, c.x, ai[o]);
                ai[o] = fma(-x.x, c.y, ai[o]);
            }
        }
        a[0] = a[4];
        a[1] = a[5];
        a[2] = a[6];
    }
    for (int k = n_w4; k < n_w; ++k) {   // the last n_w % 4 taps
        const double2 c = ws[k];
#pragma unroll
        for (int o = 0; o < XC_T; ++o) {
            const int q = XC_T * t + o + k;
            const double2 x = xs[(q & 3) * XC_PL + (q >> 2)];
            ar[o] = fma(x.x, c.x, ar[o]);
            ar[o] = fma(x.y, c.y, ar[o]);
            ai[o] = fma(x.y, c.x, ai[o]);
            ai[o] = fma(-x.x, c.y, ai[o]);
        }
    }
    XcBest m;
    m.v = 0;
    m.i = -1;
#pragma unroll
    for (int o = 0; o < XC_T; ++o) {
        const long i = i0 + XC_T * t + o;
        if (i < n_out) {
            const double v = npm::cabs_np<double>(ar[o], ai[o]);
            if (corr) corr[i] = v;
            XcBest q;
            q.v = ord_bits(v);
            q.i = i;
            m = xc_better(m, q);
        }
    }
    m = xc_block_best(m, sh);
    if (t == 0) part[blockIdx.x] = m;
}

// second stage: res[0] = peak value (f64), res[1] = its first index (int64)
__global__ __launch_bounds__(BLOCK) void k_xcorr_final(const XcBest *__restrict__ part, long n_part,
                                                       unsigned long long *__restrict__ res) {
    __shared__ XcBest sh[BLOCK / 64];
    XcBest m;
    m.v = 0;
    m.i = -1;
    for (long p = threadIdx.x; p < n_part; p += BLOCK) m = xc_better(m, part[p]);
    m = xc_block_best(m, sh);
    if (threadIdx.x == 0) {
        res[0] = m.v;
        res[1] = (unsigned long long)m.i;
    }
}

// ---- carrier loops (:287-325): one lane per candidate stream ---------------------------------
// Sequential in i and latency-bound (a sincos and, for 8PSK, an atan2 and a sin per symbol on
// the critical path); the batch is what the GPU adds.  np.exp(-1j * phase) = (cos(-phase),
// sin(-phase)); np.sign(0) = 0, np.sign(NaN) = NaN; np.round = rint.
constexpr int CR_BLOCK = 64;
__device__ __forceinline__ double np_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x)); }

__global__ __launch_bounds__(CR_BLOCK) void k_carrier(const double2 *__restrict__ syms, int n_cand, long n,
                                                      const double *__restrict__ ph0, const double *__restrict__ fr0,
                                                      const double *__restrict__ al, const int *__restrict__ kind,
                                                      double2 *__restrict__ out, double *__restrict__ fin) {
    const int c = blockIdx.x * CR_BLOCK + threadIdx.x;
    if (c >= n_cand) return;
    double phase = ph0[c], freq = fr0[c];
    const double alpha = al[c], beta = alpha * 0.1;
    const int kd = kind[c];
    const double2 *s = syms + (long)c * n;
    double2 *o = out + (long)c * n;
    for (long i = 0; i < n; ++i) {
        const double2 v = s[i];
        double sn, cs, re, im, err;
        sincos(phase, &sn, &cs);
        npm::cmul_np<double>(v.x, v.y, cs, -sn, re, im);
        o[i] = make_double2(re, im);
        if (kd == 0) {            // MDM_CR_BPSK
            err = im * np_sign(re);
        } else if (kd == 1) {     // MDM_CR_QUAD
            err = np_sign(re) * im - np_sign(im) * re;
        } else if (kd == 2) {     // MDM_CR_PSK8
            const double ps = atan2(im, re);
            const double nearest = rint(ps / 0.7853981633974483) * 0.7853981633974483;
            err = sin(ps - nearest);
        } else {
            err = (double)NAN;    // unknown kind (the host entry points reject it)
        }
        freq = freq + beta * err;
        phase = phase + (alpha * err + freq);
    }
    fin[2 * c] = phase;
    fin[2 * c + 1] = freq;
}

}  // namespace mdm
