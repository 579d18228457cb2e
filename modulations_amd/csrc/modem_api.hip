// modem_api.hip -- the C ABI (include/modem.h) over modem_kernels.hip.
//
// Per operation: one check (*_args, fir_plan), one launch (*_launch: device pointers and a stream,
// nothing checked again, no device guard) and two exported forms.  The _dev form is check -> Guard
// -> launch: stream-ordered and allocation free; tables and taps travel by value in the kernel
// arguments (no upload, no synchronisation).  The host form is check -> Guard -> Stage::run of the
// same launch: temporary device buffers on a private stream, then a synchronise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>

#include "modem.h"
#include "modem_kernels.hip"

using namespace mdm;

namespace {

// ---- kernel-order manifest ---------------------------------------
// The code object emits the non-template kernels first, as modem_kernels.hip defines them, then every
// kernel template instantiation in the order this translation unit first names it.  This never-called
// function names them all, in the order the code object has always had, so host code below cannot move a
// kernel.  A new instantiation is appended; nothing is reordered or removed while its kernel exists.
#define BOTH(k, ...) (void)k<double, ##__VA_ARGS__>, (void)k<float, ##__VA_ARGS__>;
[[maybe_unused]] void kernel_order() {
    BOTH(k_map) BOTH(k_demod) BOTH(k_fir_up, 2) BOTH(k_fir_up, 4) BOTH(k_fir_up, 8) BOTH(k_fir_up, 16)
    BOTH(k_fir_dec, 1) BOTH(k_fir_dec, 2) BOTH(k_fir_dec, 4) BOTH(k_fir_dec, 8)
    (void)k_fir<double, true>, (void)k_fir<double, false>, (void)k_fir<float, true>, (void)k_fir<float, false>;
    (void)k_absmax<double>, (void)k_quantize<double>, (void)k_absmax<float>, (void)k_quantize<float>;
    BOTH(k_mix)
    (void)k_bf_smooth<double>, (void)k_bf_flags<double>, (void)k_bf_smooth<float>, (void)k_bf_flags<float>;
}
#undef BOTH

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// What a check returns: a refusal (< 0), 0 for an empty call, which is done, or GO.  The data
// pointers (`bufs`: all there) are looked at last, so an empty call may leave them null.
constexpr int GO = 1;
int go_if(bool bufs) { return bufs ? GO : fail(MDM_EINVAL, "null buffer"); }

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? MDM_ENOMEM : MDM_EHIP,                    \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

struct Guard {
    int prev = -1;
    explicit Guard(int dev) { hipGetDevice(&prev); if (prev != dev) hipSetDevice(dev); }
    ~Guard() {
        int cur;
        hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) hipSetDevice(prev);
    }
};

// Grid for a grid-stride elementwise pass: enough blocks to fill 256 CUs several times over, never more than the work.
dim3 grid_for(long n) {
    long b = (n + BLOCK - 1) / BLOCK;
    if (b > 256L * 16) b = 256L * 16;
    return dim3((unsigned)(b < 1 ? 1 : b));
}

int launch_check(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MDM_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    return 0;
}

// The run-time f64 flag as a sample type: f(Sample<double>{}) or f(Sample<float>{}).
template <typename T> struct Sample {
    using type = T;
    static const typename C2<T>::t *in(const void *p) { return (const typename C2<T>::t *)p; }
};
template <typename F> void by_sample(int f64, F &&f) { f64 ? f(Sample<double>{}) : f(Sample<float>{}); }
// A run-time v as the one of Vs it equals: f(std::integral_constant<int, v>{}); false if it is none of them.
template <int... Vs, typename F> bool by_value(int v, F &&f) {
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// Host staging: the device guard, device buffers + private stream, freed on scope exit.  A host form declares
// its inputs, outputs and scratch (each allocates, p[] in that order), then run()s its launch: inputs up,
// launch, outputs back, synchronise.  rc is sticky: after the first failure nothing more is done.
struct Stage {
    Guard g;
    void *p[8] = {};
    struct { const void *src; void *dst; size_t bytes; } io[8] = {};
    hipStream_t st = nullptr;
    int n = 0, rc = 0;
    explicit Stage(int dev) : g(dev) { rc = init(); }
    int init() { HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); return 0; }
    int alloc(int i, size_t bytes) { HIPCHK(hipMalloc(&p[i], bytes ? bytes : 1)); return 0; }
    int h2d(int i, const void *src, size_t bytes) {
        if (src && bytes) HIPCHK(hipMemcpyAsync(p[i], src, bytes, hipMemcpyHostToDevice, st));
        return 0;
    }
    int d2h(void *dst, int i, size_t bytes) {
        if (dst && bytes) HIPCHK(hipMemcpyAsync(dst, p[i], bytes, hipMemcpyDeviceToHost, st));
        return 0;
    }
    void *buf(const void *src, void *dst, size_t bytes) {
        io[n] = {src, dst, bytes};
        if (!rc) rc = alloc(n, bytes);
        return p[n++];
    }
    template <typename T> const T *in(const T *src, size_t bytes) { return (const T *)buf(src, nullptr, bytes); }
    template <typename T> T *out(T *dst, size_t bytes) { return (T *)buf(nullptr, dst, bytes); }
    void *scratch(size_t bytes) { return buf(nullptr, nullptr, bytes); }
    template <typename F> int run(F &&launch) {
        for (int i = 0; i < n && !rc; ++i) rc = h2d(i, io[i].src, io[i].bytes);
        if (!rc) rc = launch();
        for (int i = 0; i < n && !rc; ++i) rc = d2h(io[i].dst, i, io[i].bytes);
        if (!rc) HIPCHK(hipStreamSynchronize(st));
        return rc;
    }
    ~Stage() {
        for (void *q : p)
            if (q) hipFree(q);
        if (st) hipStreamDestroy(st);
    }
};

// ---------------------------------------------------------------- mapper -----------------
// sized: look at the table's size as well.  mdm_map_dev does at once, an empty call included; mdm_map only
// when it has staged its input, so its empty call returns 0 and its null buffers are refused first.
int map_args(long n_bits, int bps, const void *table, int table_f64, bool sized, bool bufs) {
    if (n_bits < 0 || bps < 1 || bps > 8 || !table) return fail(MDM_EINVAL, "bad mapper arguments");
    if (sized && table_f64 && bps > 7) return fail(MDM_EINVAL, "complex128 mapper tables hold at most 128 points");
    return n_bits ? go_if(bufs) : 0;
}

int map_launch(hipStream_t st, const uint8_t *d_bits, long n_bits, int bps, const void *table, int table_f64,
               void *d_syms) {
    MapTable t;
    std::memset(&t, 0, sizeof t);
    std::memcpy(table_f64 ? (void *)t.d : (void *)t.f, table, (size_t)(2 << bps) * (table_f64 ? 8 : 4));
    const long n_sym = (n_bits + bps - 1) / bps, nblk = (n_sym + MAP_SPB - 1) / MAP_SPB;
    const dim3 grid((unsigned)(nblk < 256L * 8 ? nblk : 256L * 8));
    by_sample(table_f64, [&](auto s) {
        using T = typename decltype(s)::type;
        hipLaunchKernelGGL((k_map<T>), grid, dim3(BLOCK), 0, st, d_bits, n_bits, bps, n_sym, t,
                           (typename C2<T>::t *)d_syms);
    });
    return launch_check("k_map");
}

// ---------------------------------------------------------------- hard demod ---------------
int demod_args(long n_sym, int kind, int bps, const int32_t *labels, double scale, const double *cons, int nan_raises,
               bool bufs, DemodArgs &a) {
    if (n_sym < 0) return fail(MDM_EINVAL, "negative symbol count");
    std::memset(&a, 0, sizeof a);
    a.kind = kind;
    a.bps = bps;
    a.nan_raises = nan_raises ? 1 : 0;
    a.scale = scale;
    int want = 0;
    switch (kind) {
    case MDM_DEMOD_GT0: if (bps != 1) return fail(MDM_EINVAL, "GT0 demod has bps 1"); break;
    case MDM_DEMOD_QPSK: if (bps != 2) return fail(MDM_EINVAL, "QPSK demod has bps 2"); break;
    case MDM_DEMOD_PSK8: if (bps != 3) return fail(MDM_EINVAL, "8PSK demod has bps 3"); want = 8; break;
    case MDM_DEMOD_QAM_AXIS:
        // 2..8: the kernel builds a symbol's bits in eight bytes (256QAM, the mappers' M <= 256)
        if (bps < 2 || bps > 8 || bps % 2) return fail(MDM_EINVAL, "QAM demod needs an even bps of 2..8");
        a.levels = 1 << (bps / 2);
        want = a.levels;
        break;
    case MDM_DEMOD_ARGMIN:
        if (bps < 1 || (1 << bps) > ARG_MAX) return fail(MDM_EINVAL, "argmin demod supports up to 64 points");
        if (!cons) return fail(MDM_EINVAL, "argmin demod needs a constellation");
        std::memcpy(a.cons, cons, sizeof(double) * 2 * (1 << bps));
        break;
    default: return fail(MDM_EINVAL, "unknown demodulator kind");
    }
    for (int i = 0; i < want; ++i) {
        a.labels[i] = labels ? labels[i] : i;
        if (a.labels[i] < 0 || a.labels[i] >= want) return fail(MDM_EINVAL, "label table out of range");
    }
    return n_sym ? go_if(bufs) : 0;
}

// a.vec comes from the buffer the kernel writes: the caller's for mdm_demod_dev, the staging buffer for mdm_demod
int demod_launch(hipStream_t st, const void *d_syms, int sym_f64, long n_sym, DemodArgs &a, uint8_t *d_bits,
                 uint32_t *d_nan_count) {
    a.vec = ((uintptr_t)d_bits % a.bps) == 0;
    by_sample(sym_f64, [&](auto s) {
        using T = typename decltype(s)::type;
        hipLaunchKernelGGL((k_demod<T>), grid_for(n_sym), dim3(BLOCK), 0, st, s.in(d_syms), n_sym, a, d_bits,
                           d_nan_count);
    });
    return launch_check("k_demod");
}

// ---------------------------------------------------------------- FIR ----------------------
struct FirPlan { FirArgs a; bool stage; long blocks; };   // stage, blocks: the general kernel's LDS staging and grid

int fir_plan(const double *taps, long n_x, int n_taps, int up, int down, long offset, long n_out, bool bufs,
             FirPlan &p) {
    if (!taps) return fail(MDM_EINVAL, "null taps");
    if (n_x < 1 || n_taps < 1 || n_taps > TAPS_MAX || up < 1 || down < 1 || offset < 0 || n_out < 0)
        return fail(MDM_EINVAL, "bad FIR arguments");
    if ((n_out - 1) * down + offset + n_taps >= (1L << 31) || n_x * (long)up + n_taps >= (1L << 31))
        return fail(MDM_EINVAL, "FIR too long for one call (2^31 samples)");
    p.a = FirArgs{n_taps, up, down, /*per_thread*/ down == 1 ? 4 : 1, offset, n_out, n_x, /*h*/ {}};
    const long opb = (long)BLOCK * p.a.per_thread;
    const long span = ((opb - 1) * down + n_taps - 1) / up + 2;   // staged samples per block (upper bound)
    p.stage = span <= FIR_LDS;
    p.blocks = (n_out + opb - 1) / opb;
    std::memcpy(p.a.h, taps, sizeof(double) * n_taps);
    return n_out ? go_if(bufs) : 0;
}

// The grid limit is looked at where the grid is formed, and nowhere else: by mdm_fir after staging.
int fir_launch(hipStream_t st, const void *d_x, int x_f64, const FirPlan &p, double *d_out) {
    if (p.blocks > 0x7fffffffL) return fail(MDM_EINVAL, "FIR output too long");
    const FirArgs &a = p.a;
    const dim3 grid((unsigned)p.blocks), block(BLOCK);
    double2 *o = (double2 *)d_out;
    const char *what = "k_fir";
    by_sample(x_f64, [&](auto s) {
        using T = typename decltype(s)::type;
        const auto *x = s.in(d_x);
        // polyphase up-sampler / phase-major decimator for the shapes the reference uses
        if (a.down == 1 && by_value<2, 4, 8, 16>(a.up, [&](auto U) {
                const long nper = (a.n_out - 1 + a.off) / a.up + 1;
                const dim3 g2((unsigned)std::min<long>((nper + BLOCK - 1) / BLOCK, 256L * 16));
                hipLaunchKernelGGL((k_fir_up<T, decltype(U)::value>), g2, block, 0, st, x, a, o);
            }))
            what = "k_fir_up";
        else if (a.up == 1 && by_value<1, 2, 4, 8>(a.down, [&](auto D) {
                     const dim3 g2((unsigned)std::min<long>((a.n_out + BLOCK - 1) / BLOCK, 256L * 16));
                     hipLaunchKernelGGL((k_fir_dec<T, decltype(D)::value>), g2, block, 0, st, x, a, o);
                 }))
            what = "k_fir_dec";
        else if (p.stage) hipLaunchKernelGGL((k_fir<T, true>), grid, block, 0, st, x, a, o);
        else hipLaunchKernelGGL((k_fir<T, false>), grid, block, 0, st, x, a, o);
    });
    return launch_check(what);
}

// ---------------------------------------------------------------- IQ samples ---------------
int quantize_args(long n, bool bufs) {
    if (n < 1) return fail(MDM_EINVAL, "zero-size array to reduction operation maximum which has no identity");
    return go_if(bufs);
}

int quantize_launch(hipStream_t st, const void *d_sig, int sig_f64, long n, int8_t *d_iq, void *d_scratch) {
    unsigned long long *mx = (unsigned long long *)d_scratch;
    HIPCHK(hipMemsetAsync(mx, 0, 8, st));
    by_sample(sig_f64, [&](auto s) {
        using T = typename decltype(s)::type;
        hipLaunchKernelGGL((k_absmax<T>), grid_for(n), dim3(BLOCK), 0, st, s.in(d_sig), n, mx);
        hipLaunchKernelGGL((k_quantize<T>), grid_for(n), dim3(BLOCK), 0, st, s.in(d_sig), n, mx, (char2 *)d_iq);
    });
    return launch_check("k_quantize");
}

// the dequantiser's and the mixer's check
int count_args(long n, bool bufs) {
    if (n < 0) return fail(MDM_EINVAL, "negative sample count");
    return n ? go_if(bufs) : 0;
}

// vec follows the buffers the kernel uses: the caller's (mdm_iq_dequantize_dev) or the aligned staging buffers
int dequantize_launch(hipStream_t st, const uint8_t *d_raw, long n_pairs, float *d_sig) {
    const int vec = ((uintptr_t)d_raw & 15) == 0 && ((uintptr_t)d_sig & 15) == 0;
    hipLaunchKernelGGL(k_dequantize, grid_for(vec ? (n_pairs + 7) / 8 : n_pairs), dim3(BLOCK), 0, st, d_raw, n_pairs,
                       (float2 *)d_sig, vec);
    return launch_check("k_dequantize");
}

// ---------------------------------------------------------------- receive chain --------------
int mix_launch(hipStream_t st, const void *d_sig, int sig_f64, long n, long i0, const double *dc, double w, double fs,
               double *d_out) {
    const double dr = dc ? dc[0] : 0.0, di = dc ? dc[1] : 0.0;
    by_sample(sig_f64, [&](auto s) {
        using T = typename decltype(s)::type;
        hipLaunchKernelGGL((k_mix<T>), grid_for(n), dim3(BLOCK), 0, st, s.in(d_sig), n, i0, dc ? 1 : 0, (T)dr, (T)di, w,
                           fs, (double2 *)d_out);
    });
    return launch_check("k_mix");
}

int burst_args(long n, int win, long preamble_len, bool bufs) {
    if (win < 1 || win > BF_WIN_MAX) return fail(MDM_EINVAL, "smoothing window must be 1..1024 samples");
    if (n < win) return fail(MDM_EINVAL, "capture shorter than the smoothing window");
    if (preamble_len < 0) return fail(MDM_EINVAL, "negative preamble length");
    if ((n + BF_TILE - 1) / BF_TILE > 0x7fffffffL) return fail(MDM_EINVAL, "capture too long");
    return go_if(bufs);
}

int burst_launch(hipStream_t st, const void *d_sig, int sig_f64, long n, const double *dc, int win, long preamble_len,
                 double *d_smooth, void *d_result, void *d_scratch) {
    const long tiles = (n + BF_TILE - 1) / BF_TILE, half = preamble_len / 2;
    const double dr = dc ? dc[0] : 0.0, di = dc ? dc[1] : 0.0;
    unsigned long long *mx = (unsigned long long *)d_result + 1;
    int4 *tl = (int4 *)d_scratch;
    HIPCHK(hipMemsetAsync(d_result, 0, 16, st));
    const dim3 grid((unsigned)tiles);
    by_sample(sig_f64, [&](auto s) {
        using T = typename decltype(s)::type;
        hipLaunchKernelGGL((k_bf_smooth<T>), grid, dim3(BLOCK), 0, st, s.in(d_sig), n, (T)dr, (T)di, win, d_smooth, mx);
        hipLaunchKernelGGL((k_bf_flags<T>), grid, dim3(BLOCK), 0, st, s.in(d_sig), n, (T)dr, (T)di, win, half, mx, tl);
    });
    hipLaunchKernelGGL(k_bf_scan, dim3(1), dim3(BLOCK), 0, st, tl, tiles, n, preamble_len, half,
                       (long long *)d_result);
    return launch_check("k_bf_scan");
}

int xcorr_args(long n_region, int n_w, bool bufs) {
    if (n_w < 1 || n_w > XC_NW) return fail(MDM_EINVAL, "sync waveform must have 1..1024 taps");
    if (n_region < n_w) return fail(MDM_EINVAL, "search region shorter than the sync waveform");
    if ((n_region - n_w + XC_OPB) / XC_OPB > 0x7fffffffL) return fail(MDM_EINVAL, "search region too long");
    return go_if(bufs);
}

int xcorr_launch(hipStream_t st, const double *d_region, long n_region, const double *d_w, int n_w, double *d_corr,
                 void *d_result, void *d_scratch) {
    const long n_out = n_region - n_w + 1, blocks = (n_out + XC_OPB - 1) / XC_OPB;
    hipLaunchKernelGGL(k_xcorr, dim3((unsigned)blocks), dim3(BLOCK), 0, st, (const double2 *)d_region, n_region,
                       (const double2 *)d_w, n_w, n_out, d_corr, (XcBest *)d_scratch);
    hipLaunchKernelGGL(k_xcorr_final, dim3(1), dim3(BLOCK), 0, st, (const XcBest *)d_scratch, blocks,
                       (unsigned long long *)d_result);
    return launch_check("k_xcorr");
}

// host_kind: mdm_carrier's detector kinds, which it can read and so checks; mdm_carrier_dev's are on the
// device (nullptr here) and go to the kernel unchecked.
int carrier_args(int n_cand, long n, bool bufs, const int32_t *host_kind) {
    if (n_cand < 0 || n < 0) return fail(MDM_EINVAL, "negative carrier batch or length");
    if (n_cand == 0) return 0;
    if (!bufs) return go_if(bufs);
    for (int c = 0; host_kind && c < n_cand; ++c)
        if (host_kind[c] < MDM_CR_BPSK || host_kind[c] > MDM_CR_PSK8)
            return fail(MDM_EINVAL, "unknown carrier detector kind");
    return GO;
}

int carrier_launch(hipStream_t st, const double *d_syms, int n_cand, long n, const double *d_phase,
                   const double *d_freq, const double *d_alpha, const int32_t *d_kind, double *d_out, double *d_final) {
    hipLaunchKernelGGL(k_carrier, dim3((unsigned)((n_cand + CR_BLOCK - 1) / CR_BLOCK)), dim3(CR_BLOCK), 0, st,
                       (const double2 *)d_syms, n_cand, n, d_phase, d_freq, d_alpha, d_kind, (double2 *)d_out, d_final);
    return launch_check("k_carrier");
}

}  // namespace

extern "C" {

const char *mdm_last_error(void) { return g_err.c_str(); }

int mdm_map_dev(int device, const uint8_t *d_bits, long n_bits, int bps, const void *table, int table_f64,
                void *d_syms, void *stream) {
    if (int rc = map_args(n_bits, bps, table, table_f64, true, d_bits && d_syms); rc <= 0) return rc;
    Guard g(device);
    return map_launch((hipStream_t)stream, d_bits, n_bits, bps, table, table_f64, d_syms);
}

int mdm_map(int device, const uint8_t *bits, long n_bits, int bps, const void *table, int table_f64, void *syms) {
    if (int rc = map_args(n_bits, bps, table, table_f64, false, bits && syms); rc <= 0) return rc;
    Stage s(device);
    const uint8_t *d_bits = s.in(bits, (size_t)n_bits);
    void *d_syms = s.out(syms, (size_t)((n_bits + bps - 1) / bps) * (table_f64 ? 16 : 8));
    return s.run([&] {
        if (int rc = map_args(n_bits, bps, table, table_f64, true, true); rc < 0) return rc;
        return map_launch(s.st, d_bits, n_bits, bps, table, table_f64, d_syms);
    });
}

int mdm_demod_dev(int device, int kind, const void *d_syms, int sym_f64, long n_sym, int bps, const int32_t *labels,
                  double scale, const double *cons, int nan_raises, uint8_t *d_bits, uint32_t *d_nan_count,
                  void *stream) {
    DemodArgs a;
    if (int rc = demod_args(n_sym, kind, bps, labels, scale, cons, nan_raises, d_syms && d_bits, a); rc <= 0) return rc;
    Guard g(device);
    return demod_launch((hipStream_t)stream, d_syms, sym_f64, n_sym, a, d_bits, d_nan_count);
}

int mdm_demod(int device, int kind, const void *syms, int sym_f64, long n_sym, int bps, const int32_t *labels,
              double scale, const double *cons, int nan_raises, uint8_t *bits) {
    DemodArgs a;
    if (int rc = demod_args(n_sym, kind, bps, labels, scale, cons, nan_raises, syms && bits, a); rc <= 0) return rc;
    uint32_t nans = 0;
    Stage s(device);
    const void *d_syms = s.in(syms, (size_t)n_sym * (sym_f64 ? 16 : 8));
    uint8_t *d_bits = s.out(bits, (size_t)n_sym * bps);
    uint32_t *d_nans = s.out(&nans, 4);
    int rc = s.run([&] {
        HIPCHK(hipMemsetAsync(s.p[2], 0, 4, s.st));
        return demod_launch(s.st, d_syms, sym_f64, n_sym, a, d_bits, d_nans);
    });
    if (!rc && nans) return fail(MDM_ENAN, "cannot convert float NaN to integer");
    return rc;
}

int mdm_fir_dev(int device, const void *d_x, int x_f64, long n_x, const double *taps, int n_taps, int up, int down,
                long offset, long n_out, double *d_out, void *stream) {
    FirPlan p;
    if (int rc = fir_plan(taps, n_x, n_taps, up, down, offset, n_out, d_x && d_out, p); rc <= 0) return rc;
    Guard g(device);
    return fir_launch((hipStream_t)stream, d_x, x_f64, p, d_out);
}

int mdm_fir(int device, const void *x, int x_f64, long n_x, const double *taps, int n_taps, int up, int down,
            long offset, long n_out, double *out) {
    FirPlan p;
    if (int rc = fir_plan(taps, n_x, n_taps, up, down, offset, n_out, x && out, p); rc <= 0) return rc;
    Stage s(device);
    const void *d_x = s.in(x, (size_t)n_x * (x_f64 ? 16 : 8));
    double *d_out = s.out(out, (size_t)n_out * 16);
    return s.run([&] { return fir_launch(s.st, d_x, x_f64, p, d_out); });
}

int mdm_iq_quantize_dev(int device, const void *d_sig, int sig_f64, long n, int8_t *d_iq, void *d_scratch,
                        void *stream) {
    if (int rc = quantize_args(n, d_sig && d_iq && d_scratch); rc <= 0) return rc;
    Guard g(device);
    return quantize_launch((hipStream_t)stream, d_sig, sig_f64, n, d_iq, d_scratch);
}

int mdm_iq_quantize(int device, const void *sig, int sig_f64, long n, int8_t *iq) {
    if (int rc = quantize_args(n, sig && iq); rc <= 0) return rc;
    Stage s(device);
    const void *d_sig = s.in(sig, (size_t)n * (sig_f64 ? 16 : 8));
    int8_t *d_iq = s.out(iq, (size_t)n * 2);
    void *d_max = s.scratch(8);
    return s.run([&] { return quantize_launch(s.st, d_sig, sig_f64, n, d_iq, d_max); });
}

int mdm_iq_dequantize_dev(int device, const uint8_t *d_raw, long n_pairs, float *d_sig, void *stream) {
    if (int rc = count_args(n_pairs, d_raw && d_sig); rc <= 0) return rc;
    Guard g(device);
    return dequantize_launch((hipStream_t)stream, d_raw, n_pairs, d_sig);
}

int mdm_iq_dequantize(int device, const uint8_t *raw, long n_pairs, float *sig) {
    if (int rc = count_args(n_pairs, raw && sig); rc <= 0) return rc;
    Stage s(device);
    const uint8_t *d_raw = s.in(raw, (size_t)n_pairs * 2);
    float *d_sig = s.out(sig, (size_t)n_pairs * 8);
    return s.run([&] { return dequantize_launch(s.st, d_raw, n_pairs, d_sig); });
}

int mdm_mix_dev(int device, const void *d_sig, int sig_f64, long n, long i0, const double *dc, double w, double fs,
                double *d_out, void *stream) {
    if (int rc = count_args(n, d_sig && d_out); rc <= 0) return rc;
    Guard g(device);
    return mix_launch((hipStream_t)stream, d_sig, sig_f64, n, i0, dc, w, fs, d_out);
}

int mdm_mix(int device, const void *sig, int sig_f64, long n, long i0, const double *dc, double w, double fs,
            double *out) {
    if (int rc = count_args(n, sig && out); rc <= 0) return rc;
    Stage s(device);
    const void *d_sig = s.in(sig, (size_t)n * (sig_f64 ? 16 : 8));
    double *d_out = s.out(out, (size_t)n * 16);
    return s.run([&] { return mix_launch(s.st, d_sig, sig_f64, n, i0, dc, w, fs, d_out); });
}

int mdm_burst_find_dev(int device, const void *d_sig, int sig_f64, long n, const double *dc, int win,
                       long preamble_len, double *d_smooth, void *d_result, void *d_scratch, void *stream) {
    if (int rc = burst_args(n, win, preamble_len, d_sig && d_result && d_scratch); rc <= 0) return rc;
    Guard g(device);
    return burst_launch((hipStream_t)stream, d_sig, sig_f64, n, dc, win, preamble_len, d_smooth, d_result, d_scratch);
}

int mdm_burst_find(int device, const void *sig, int sig_f64, long n, const double *dc, int win, long preamble_len,
                   long long *burst_start, double *max_power, double *smooth) {
    if (int rc = burst_args(n, win, preamble_len, sig && burst_start); rc <= 0) return rc;
    long long r[2];
    Stage s(device);
    const void *d_sig = s.in(sig, (size_t)n * (sig_f64 ? 16 : 8));
    void *d_res = s.out(r, 16), *d_tl = s.scratch((size_t)((n + BF_TILE - 1) / BF_TILE) * 16);
    double *d_smooth = smooth ? s.out(smooth, (size_t)n * 8) : nullptr;
    const int rc =
        s.run([&] { return burst_launch(s.st, d_sig, sig_f64, n, dc, win, preamble_len, d_smooth, d_res, d_tl); });
    if (rc) return rc;
    *burst_start = r[0];
    if (max_power) std::memcpy(max_power, &r[1], 8);
    return 0;
}

int mdm_xcorr_peak_dev(int device, const double *d_region, long n_region, const double *d_w, int n_w, double *d_corr,
                       void *d_result, void *d_scratch, void *stream) {
    if (int rc = xcorr_args(n_region, n_w, d_region && d_w && d_result && d_scratch); rc <= 0) return rc;
    Guard g(device);
    return xcorr_launch((hipStream_t)stream, d_region, n_region, d_w, n_w, d_corr, d_result, d_scratch);
}

int mdm_xcorr_peak(int device, const double *region, long n_region, const double *w, int n_w, double *corr,
                   long long *argmax, double *peak) {
    if (int rc = xcorr_args(n_region, n_w, region && w && argmax); rc <= 0) return rc;
    const long n_out = n_region - n_w + 1;
    long long r[2];
    Stage s(device);
    const double *d_region = s.in(region, (size_t)n_region * 16), *d_w = s.in(w, (size_t)n_w * 16);
    void *d_result = s.out(r, 16), *d_part = s.scratch((size_t)((n_out + XC_OPB - 1) / XC_OPB) * 16);
    double *d_corr = corr ? s.out(corr, (size_t)n_out * 8) : nullptr;
    const int rc = s.run([&] { return xcorr_launch(s.st, d_region, n_region, d_w, n_w, d_corr, d_result, d_part); });
    if (rc) return rc;
    if (peak) std::memcpy(peak, &r[0], 8);
    *argmax = r[1];
    return 0;
}

int mdm_carrier_dev(int device, const double *d_syms, int n_cand, long n, const double *d_phase, const double *d_freq,
                    const double *d_alpha, const int32_t *d_kind, double *d_out, double *d_final, void *stream) {
    const bool bufs = d_phase && d_freq && d_alpha && d_kind && d_final && (!n || (d_syms && d_out));
    if (int rc = carrier_args(n_cand, n, bufs, nullptr); rc <= 0) return rc;
    Guard g(device);
    return carrier_launch((hipStream_t)stream, d_syms, n_cand, n, d_phase, d_freq, d_alpha, d_kind, d_out, d_final);
}

int mdm_carrier(int device, const double *syms, int n_cand, long n, const double *phase, const double *freq,
                const double *alpha, const int32_t *kind, double *out, double *final_state) {
    const bool bufs = phase && freq && alpha && kind && final_state && (!n || (syms && out));
    if (int rc = carrier_args(n_cand, n, bufs, kind); rc <= 0) return rc;
    const size_t sb = (size_t)n_cand * (size_t)n * 16, pb = (size_t)n_cand * 8;
    Stage s(device);
    const double *d_syms = s.in(syms, sb), *d_ph = s.in(phase, pb), *d_fr = s.in(freq, pb), *d_al = s.in(alpha, pb);
    const int32_t *d_kind = s.in(kind, pb / 2);
    double *d_out = s.out(out, sb), *d_fin = s.out(final_state, 2 * pb);
    return s.run([&] { return carrier_launch(s.st, d_syms, n_cand, n, d_ph, d_fr, d_al, d_kind, d_out, d_fin); });
}

}  // extern "C"
