// tdec_demap_kernels.hip -- gfx950 kernels of the soft demapper:
// the max-log demapper (compute_llr), flat and into the decoder's planes, the log-MAP
// demapper, the noise-variance estimator, the flat-fading equaliser, the demapper
// prologue of the fused demap + decode kernel, and the self-tests of the exact shortcuts.
// Included by tdec_api.hip after tdec_kernels.hip, whose tile layout, launch constants
// and turbo_decode_tiles it uses.
namespace tdec {

// ---- soft demapper (compute_llr, test_sdr_with_coding.py:200-225) -----------------
// numpy's complex |z|: npmath.hip
using npm::cabs_np;

struct DemapCfg {
    int M, div_f32, sign;
    double nv;                 // max(noise_var, 0.005) already applied (:202)
    int sep;                   // 1: separable square QAM grid (per-axis levels follow the points);
                               // 2: and each axis a Gray-labelled uniform PAM (position-ordered levels follow)
    int nv_fast;               // nv in [2^-8, 2^16]: the unscaled f32 / f64 division (dm_fast)
};
__host__ __device__ inline int dm_nv_fast(double nv) { return nv >= 0x1p-8 && nv <= 0x1p16; }
// Per-row and per-symbol noise variance (ROWNV): the demap kernels'
// last argument.  ROWNV 0: empty, the scalar kernels, whose DemapCfg carries the launch's
// one value; 1: a device vector, one value per row of [B][S] symbols; 2: a device array,
// one value per symbol.  Each thread forms its symbol's configuration from it with the
// host's own expressions (demap_cfg / demap_lm_scale, tdec_demap_api.hip), so row r (symbol
// (r, s)) is what the scalar launch gives it with nvs[r] (nvs[r * S + s]).
template <int ROWNV> struct RowNv {};
template <> struct RowNv<1> {
    const double *nvs;         // device, [B]
    long S;                    // symbols per row (the flat kernels' row = symbol / S)
};
template <> struct RowNv<2> {
    const double *nvs;         // device, [B][S]
    long S;                    // symbols per row
};
// nv_at: the value of flat symbol s (the flat kernels: row s / S, symbol s % S) or of symbol
// s of codeword cw (the tile kernels; cw < B, s < S).  One 8-byte load per symbol: with
// ROWNV 2 consecutive threads read consecutive addresses within a row, and the symbols of
// a couple that straddles two of them each take their own.
__device__ __forceinline__ double nv_at(const RowNv<1> &rn, long s) { return rn.nvs[s / rn.S]; }
__device__ __forceinline__ double nv_at(const RowNv<2> &rn, long s) { return rn.nvs[s]; }
__device__ __forceinline__ double nv_at(const RowNv<1> &rn, long cw, long) { return rn.nvs[cw]; }
__device__ __forceinline__ double nv_at(const RowNv<2> &rn, long cw, long s) { return rn.nvs[cw * rn.S + s]; }
__device__ __forceinline__ DemapCfg row_cfg(const DemapCfg &c, double x) {
    DemapCfg r = c;
    r.nv = (0.005 > x) ? 0.005 : x;   // a NaN x stays NaN, as on the host
    r.nv_fast = dm_nv_fast(r.nv);
    return r;
}
// cfg_at(c, rn, s) / cfg_at(c, rn, cw, s): the symbol's configuration in every mode, the
// launch's own c for the scalar kernels.  lm_scale_at: the log-MAP scale that goes with it,
// the launch's for the scalar kernels.
template <class... I> __device__ __forceinline__ const DemapCfg &cfg_at(const DemapCfg &c, const RowNv<0> &, I...) {
    return c;
}
template <int ROWNV, class... I>
__device__ __forceinline__ DemapCfg cfg_at(const DemapCfg &c, const RowNv<ROWNV> &rn, I... i) {
    return row_cfg(c, nv_at(rn, i...));
}
template <typename T> __device__ __forceinline__ T lm_scale_at(const DemapCfg &, const RowNv<0> &, T launch) {
    return launch;
}
template <typename T, int ROWNV> __device__ __forceinline__ T lm_scale_at(const DemapCfg &rc, const RowNv<ROWNV> &, T) {
    return (T)(1.0 / (rc.nv * 0.693147180559945309417));
}
// LDS table: 2*M point coordinates (+ 2 * 2^(bps/2) axis levels in label order; for a
// uniform grid labelled through gray[], sep == 2, + the levels in position order, 4
// parameters and the 2 * K * 2^K neighbour positions of sym_llrs_gray)
constexpr int DM_TAB = 768;

// The unscaled sequences (dm_fast): the compiler's own f64 division and square root
// sequences without their range scaling, where the scaling is provably the
// identity -- the same instructions on the same values, so the same bits:
//   a / b: v_div_scale (identity) -> r = v_rcp_f64(b), two Newton steps
//   r += r * (1 - b r), q = a r, rem = a - b q, q += rem r (v_div_fmas without its
//   2^64 scale), v_div_fixup (identity for finite nonzero operands and a normal
//   quotient); v_div_scale scales only for a denormal or huge denominator, a
//   numerator below 2^-969, a quotient below 2^-1022 or an exponent difference
//   >= 768;
//   sqrt(x), x in [1, 2]: y = v_rsq_f64(x), g = x y, h = y / 2, one Goldschmidt
//   step and two corrections (the 2^256 pre-scale applies below 2^-767 and the
//   zero / inf class select never fires).
// Outside those ranges the compiler's sequences run (a branch no lane takes on
// ordinary symbols).  tdec_selftest 4 compares both against the compiler's
// sequences on random operands over the ranges the demapper meets.
// BPSK .. 16QAM (measured faster, profiles/r05/demap_ab/); the 64 / 256QAM kernels
// keep the compiler's sequences (their registers grow past an occupancy step)
__host__ __device__ constexpr bool dm_fast(int bps) { return bps <= 4; }
__device__ __forceinline__ double rcp_nr64(double b) {   // v_div_scale-free reciprocal of the division sequence
    double r = __builtin_amdgcn_rcp(b);
    r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
    return __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
}
__device__ __forceinline__ double div_nr64(double a, double b, double r) {   // a / b given r = rcp_nr64(b)
    const double q = a * r;
    return __builtin_fma(__builtin_fma(-b, q, a), r, q);
}
// The f32 division the same way (v_div_scale_f32 scales for a denormal or huge
// denominator, a numerator below 2^-104, a denormal quotient or an exponent
// difference >= 96): r = v_rcp_f32(b), one Newton step, q = a r, two corrections
// (the second is v_div_fmas_f32 without its scale).
__device__ __forceinline__ float rcp_nr32(float b) {
    const float r = __builtin_amdgcn_rcpf(b);
    return __builtin_fmaf(__builtin_fmaf(-b, r, 1.0f), r, r);
}
__device__ __forceinline__ float div_nr32(float a, float b, float r) {   // a / b given r = rcp_nr32(b)
    float q = a * r;
    q = __builtin_fmaf(__builtin_fmaf(-b, q, a), r, q);
    return __builtin_fmaf(__builtin_fmaf(-b, q, a), r, q);
}
__device__ __forceinline__ double sqrt_1_2_64(double x) {   // sqrt(x) for x in [1, 2]
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    double d = __builtin_fma(-g, g, x);
    h = __builtin_fma(h, r, h);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
// One LLR from the two per-half minima (:219-225): NaN propagates, then the
// division by the noise variance, the +-30 clip and the caller's sign.
// PRE: the caller has checked nv_fast and that |diff| lies in the unscaled range
// (sym_llrs_pairs16), so the unscaled division runs without a per-LLR test.
// F32OUT (PRE only): the caller keeps the LLR as f32 (the plane kernels), so the
// f64 quotient is rounded first and clipped / negated in f32: the same value, since
// +-30 are f32 values, rounding is monotone and the quotient is finite here.
template <typename T, bool FAST = false, bool PRE = false, bool F32OUT = false>
__device__ __forceinline__ double llr_from_diff(T diff, const DemapCfg &c) {
    if constexpr (PRE) {
        if (sizeof(T) == 4 && c.div_f32) {
            const float fn = (float)c.nv;
            float q = div_nr32((float)diff, fn, rcp_nr32(fn));
            q = q < -30.0f ? -30.0f : (q > 30.0f ? 30.0f : q);   // finite: no NaN test
            return (double)(c.sign < 0 ? -q : q);
        }
        if constexpr (F32OUT) {
            const float f = __builtin_amdgcn_fmed3f((float)div_nr64((double)diff, c.nv, rcp_nr64(c.nv)), -30.0f, 30.0f);
            return (double)(c.sign < 0 ? -f : f);
        }
        double v = div_nr64((double)diff, c.nv, rcp_nr64(c.nv));
        v = v < -30.0 ? -30.0 : (v > 30.0 ? 30.0 : v);
        return c.sign < 0 ? -v : v;
    }
    if (sizeof(T) == 4 && c.div_f32) {
        // the f32 quotient clipped and negated in f32: the same values as in f64
        // (f32 -> f64 is exact and so are the +-30 clip and the negation)
        // dm_fast: nv in [2^-8, 2^16], |diff| in [2^-90, 2^60]: nothing scaled
        const float fd = (float)diff, fn = (float)c.nv, af = fabsf(fd);
        float q = FAST && c.nv_fast && af >= 0x1p-90f && af <= 0x1p60f ? div_nr32(fd, fn, rcp_nr32(fn))
                                                                                  : fd / fn;
        if (q == q) q = q < -30.0f ? -30.0f : (q > 30.0f ? 30.0f : q);   // np.clip(llr, -30, 30)
        return (double)(c.sign < 0 ? -q : q);
    }
    double v;
    const double dd = (double)diff, ad = fabs(dd);
    // dm_fast: nv in [2^-8, 2^16] (host flag) and |diff| in [2^-900, 2^600]:
    // no operand or quotient the division sequence would scale (zero, whose sign
    // v_div_fixup sets, NaN and inf take the compiler's division)
    if (FAST && c.nv_fast && ad >= 0x1p-900 && ad <= 0x1p600) v = div_nr64(dd, c.nv, rcp_nr64(c.nv));
    else v = dd / c.nv;
    if (v == v) v = v < -30.0 ? -30.0 : (v > 30.0 ? 30.0 : v);
    return c.sign < 0 ? -v : v;
}
template <typename T, bool FAST = false> __device__ __forceinline__ double llr_of(T lo, T hi, const DemapCfg &c) {
    return llr_from_diff<T, FAST>(lo - hi, c);
}

// Square QAM whose label splits into K I-bits and K Q-bits (16/64/256QAM of
// sdr_modem.py:142-220): point (a, q) = levI[a] + j levQ[q].  The minimum of
// numpy's |s - c|^2 over a bit-half is taken at the point nearest in plain
// dx^2 + dy^2 (computed from the same rounded differences) unless two points of
// the half are within a relative 64 ulp of each other: that point is found per
// axis (2^K levels instead of 2^(2K) points) and only the 2*BPS candidates get
// numpy's distance.  Near ties, non-finite input or underflow return false and
// the caller runs the full scan, so the result is the scan's, bit for bit.
//
// The gap test may be stricter than needed, never looser (a stricter test only
// sends more symbols to the exact scan): one tolerance from the largest
// candidate distance serves every half, and once every gap is strictly positive
// the argmin of a half is unique, so min / max order statistics and any
// tie-break give the same candidates.  Inside the fast path every difference is
// finite, so |z| skips numpy's inf / NaN rules (cabs_fin).
// numpy's |z| (npm::cabs_np) for finite re, im: the same operations without the
// inf / NaN selects; f32's square root of fma(r, r, 1) in [1, 2] as the raw
// v_sqrt_f32 plus the compiler's own +-1 ulp correction (its input scaling and
// zero / inf class test are identities on [1, 2]), so bit-identical to sqrtf.
template <typename T> __device__ __forceinline__ T sqrt_1_2(T x) {
    if constexpr (sizeof(T) == 8) {
        return sqrt(x);
    } else {
        const float r = __builtin_amdgcn_sqrtf(x);
        const float dn = __int_as_float(__float_as_int(r) - 1), up = __int_as_float(__float_as_int(r) + 1);
        const float rd = __builtin_fmaf(-dn, r, x), ru = __builtin_fmaf(-up, r, x);
        const float t = rd <= 0.0f ? dn : r;
        return ru > 0.0f ? up : t;
    }
}
template <typename T, bool FAST = false, bool PRE = false> __device__ __forceinline__ T cabs_fin(T re, T im) {
    re = fabs(re);
    im = fabs(im);
    const T larger = re > im ? re : im;
    const T smaller = im < re ? im : re;
    if constexpr (sizeof(T) == 8 && FAST) {
        // larger in [2^-800, 2^800]: no scaling of the denominator; a numerator or
        // quotient small enough to be scaled gives ratio < 2^-169, where
        // fma(ratio, ratio, 1) is 1 whatever its last bits
        if (PRE || (larger >= 0x1p-800 && larger <= 0x1p800)) {
            const double ratio = div_nr64(smaller, larger, rcp_nr64(larger));
            return sqrt_1_2_64(__builtin_fma(ratio, ratio, 1.0)) * larger;
        }
    }
    if constexpr (sizeof(T) == 4 && FAST) {
        // larger in [2^-80, 2^100]: likewise, a scaled numerator or quotient gives
        // ratio < 2^-24 (fma(ratio, ratio, 1) = 1 in f32 below 2^-12.5)
        if (PRE || (larger >= 0x1p-80f && larger <= 0x1p100f)) {
            const float ratio = div_nr32(smaller, larger, rcp_nr32(larger));
            return sqrt_1_2<float>(__builtin_fmaf(ratio, ratio, 1.0f)) * larger;
        }
    }
    const T ratio = larger != (T)0 ? smaller / larger : (T)0;
    return sqrt_1_2<T>(fma(ratio, ratio, (T)1)) * larger;
}

// 16QAM (nv_fast): the per-axis search below for K = 2 in closed
// form, carrying the differences instead of level indices.  Every bit-half holds
// two levels ({0, 1} / {2, 3} for the label's high bit, {0, 2} / {1, 3} for its
// low bit), so its nearest / second nearest / first argmin are a min / max /
// compare of the pair; the axis' nearest is the nearer of the high bit's pair
// minima (ties to the lower labels, as the streamed first-minimum rule) and its
// second nearest min(max of those minima, min of the pair maxima): the same
// values, so the same gap test.  The candidates' differences s - level are the
// ones the search formed (the streamed form forms them again from the indices).
// One range test per symbol replaces the unscaled sequences' per-call tests:
// every candidate's larger |difference| lies between the axes' nearest
// differences and the largest difference, and every LLR numerator below twice
// its square; a symbol outside declines (its LLRs come from the full chain).
template <typename T, bool F32OUT = false>
__device__ __forceinline__ bool sym_llrs_pairs16(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[4]) {
    constexpr bool F32 = sizeof(T) == 4;
    if (!(isfinite(sr) && isfinite(si))) return false;
    const T *lev_i = cons + 2 * 16, *lev_q = lev_i + 4;
    const T inf = (T)INFINITY;
    const T eps = F32 ? (T)3.8e-6 : (T)7.2e-15, tau = F32 ? (T)1e-30 : (T)1e-290;
    T dn[2], dc[2][2], all1[2];
    bool vn[2][2];
    T gap = inf, top = (T)0, hi = (T)0, dmax = (T)0;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        const T s = ax ? si : sr;
        const T *lev = ax ? lev_q : lev_i;
        T d[4], d2[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            d[a] = s - lev[a];
            d2[a] = d[a] * d[a];
            dmax = fmax(dmax, fabs(d[a]));
        }
        T b1[2][2], b2[2][2], bd[2][2];
        bool lt[2][2];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int p = b ? v : 2 * v, q = b ? v + 2 : 2 * v + 1;   // the half's two levels, p < q
                lt[b][v] = d2[q] < d2[p];
                b1[b][v] = fmin(d2[p], d2[q]);
                b2[b][v] = fmax(d2[p], d2[q]);
                bd[b][v] = lt[b][v] ? d[q] : d[p];
                gap = fmin(gap, b2[b][v] - b1[b][v]);
                top = fmax(top, b1[b][v]);
                hi = fmax(hi, b2[b][v]);
            }
        const T a1 = fmin(b1[0][0], b1[0][1]), a2 = fmin(fmax(b1[0][0], b1[0][1]), fmin(b2[0][0], b2[0][1]));
        gap = fmin(gap, a2 - a1);
        hi = fmax(hi, a2);
        all1[ax] = a1;
        const bool hv = b1[0][1] < b1[0][0];                 // the nearest level's label bits
        const bool lv = hv ? lt[0][1] : lt[0][0];
        dn[ax] = hv ? bd[0][1] : bd[0][0];
        dc[ax][0] = hv ? bd[0][0] : bd[0][1];               // nearest with the other high bit
        dc[ax][1] = lv ? bd[1][0] : bd[1][1];               // nearest with the other low bit
        vn[ax][0] = hv;
        vn[ax][1] = lv;
    }
    const T tol = eps * (top + fmax(all1[0], all1[1])) + tau;
    const T l0 = fmax(fabs(dn[0]), fabs(dn[1]));
    if (!(hi < inf && gap > tol && l0 >= (F32 ? (T)0x1p-80f : (T)0x1p-800) && dmax <= (F32 ? (T)0x1p29f : (T)0x1p290)))
        return false;
    const T an = cabs_fin<T, true, true>(dn[0], dn[1]);
    const T dq = an * an;
    const T lo = F32 ? (c.div_f32 ? (T)0x1p-90f : (T)0x1p-149f) : (T)0x1p-900;
    T diff[4];
#pragma unroll
    for (int ax = 0; ax < 2; ++ax)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const T a = ax ? cabs_fin<T, true, true>(dn[0], dc[1][b]) : cabs_fin<T, true, true>(dc[0][b], dn[1]);
            const T ao = a * a;
            diff[ax * 2 + b] = vn[ax][b] ? ao - dq : dq - ao;   // m[0] - m[1], m[vn] = dn
        }
    if (!(fmin(fmin(fabs(diff[0]), fabs(diff[1])), fmin(fabs(diff[2]), fabs(diff[3]))) >= lo)) return false;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = llr_from_diff<T, true, true, F32OUT>(diff[k], c);
    return true;
}

template <typename T, int BPS, bool F32OUT = false>
__device__ __forceinline__ bool sym_llrs_sep(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[BPS]) {
    constexpr int K = BPS / 2, L = 1 << K;
    const T *lev_i = cons + 2 * (1 << BPS), *lev_q = lev_i + L;
    const T inf = (T)INFINITY;
    const T eps = sizeof(T) == 4 ? (T)3.8e-6 : (T)7.2e-15, tau = sizeof(T) == 4 ? (T)1e-30 : (T)1e-290;
    if constexpr (K == 2 && dm_fast(BPS)) {
        if (c.nv_fast) return sym_llrs_pairs16<T, F32OUT>(sr, si, cons, c, out);
    }
    T all1[2], all2[2], b1[2][K][2], b2[2][K][2];   // nearest / second nearest: axis, bit-halves
    int arg[2][K][2], allarg[2];
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        const T s = ax ? si : sr;
        const T *lev = ax ? lev_q : lev_i;
        // streamed over the levels: nearest / second nearest of the axis and of
        // each bit-half (a NaN distance is dropped by fmin / fmax; then every
        // distance of the axis is NaN, the minima stay inf and the test below
        // fails)
        T m1 = inf, m2 = inf;
        int am = 0;
#pragma unroll
        for (int b = 0; b < K; ++b)
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                b1[ax][b][v] = b2[ax][b][v] = inf;
                arg[ax][b][v] = 0;
            }
#pragma unroll
        for (int a = 0; a < L; ++a) {
            const T d = s - lev[a];
            const T d2 = d * d;
            m2 = fmin(m2, fmax(m1, d2));
            am = d2 < m1 ? a : am;
            m1 = fmin(m1, d2);
#pragma unroll
            for (int b = 0; b < K; ++b) {
                const int v = (a >> (K - 1 - b)) & 1;
                b2[ax][b][v] = fmin(b2[ax][b][v], fmax(b1[ax][b][v], d2));
                arg[ax][b][v] = d2 < b1[ax][b][v] ? a : arg[ax][b][v];
                b1[ax][b][v] = fmin(b1[ax][b][v], d2);
            }
        }
        all1[ax] = m1;
        all2[ax] = m2;
        allarg[ax] = am;
    }
    T gap = fmin(all2[0] - all1[0], all2[1] - all1[1]), top = (T)0, hi = fmax(all2[0], all2[1]);
#pragma unroll
    for (int ax = 0; ax < 2; ++ax)
#pragma unroll
        for (int b = 0; b < K; ++b)
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                gap = fmin(gap, b2[ax][b][v] - b1[ax][b][v]);
                top = fmax(top, b1[ax][b][v]);
                hi = fmax(hi, b2[ax][b][v]);
            }
    // every gap above the tolerance of the largest candidate distance
    // (best + the other axis' nearest), every second nearest finite
    const T tol = eps * (top + fmax(all1[0], all1[1])) + tau;
    if (!(hi < inf && gap > tol)) return false;
    // The half holding the overall nearest point has that point as its
    // candidate, so its distance is shared by every bit: BPS + 1 numpy
    // distances instead of 2 * BPS.
    const T an = cabs_fin<T, dm_fast(BPS)>(sr - lev_i[allarg[0]], si - lev_q[allarg[1]]);
    const T dn = an * an;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax)
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const int vn = (allarg[ax] >> (K - 1 - b)) & 1, vo = vn ^ 1;
            const int ia = ax ? allarg[0] : arg[0][b][vo], iq = ax ? arg[1][b][vo] : allarg[1];
            const T a = cabs_fin<T, dm_fast(BPS)>(sr - lev_i[ia], si - lev_q[iq]);
            const T ao = a * a;
            out[ax * K + b] = llr_from_diff<T, dm_fast(BPS)>(vn ? ao - dn : dn - ao, c);   // m[0] - m[1], m[vn] = dn
        }
    return true;
}

// All BPS LLRs of one symbol, reference sign (positive -> bit 1) unless
// c.sign < 0.  Streams over the M points keeping a running min per bit and
// label value, so no distance array is materialised.
template <typename T, int BPS, bool FIN, int M = (1 << BPS), int UNROLL = (M <= 16 ? M : 8)>
__device__ __forceinline__ void sym_llrs_scan(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[BPS]) {
    T m0[BPS], m1[BPS];
    bool n0[BPS], n1[BPS];
#pragma unroll
    for (int b = 0; b < BPS; ++b) {
        m0[b] = m1[b] = (T)INFINITY;
        n0[b] = n1[b] = false;
    }
    // M is the full label space; a table with fewer points (c.M < M) stops early.
#pragma unroll UNROLL
    for (int m = 0; m < M; ++m) {
        if (M > 2 && m >= c.M) break;
        const T a = FIN ? cabs_fin<T, dm_fast(BPS)>(sr - cons[2 * m], si - cons[2 * m + 1]) : cabs_np<T>(sr - cons[2 * m], si - cons[2 * m + 1]);
        const T v = a * a;                     // np.abs(s - constellation) ** 2
        const bool vn = v != v;
#pragma unroll
        for (int b = 0; b < BPS; ++b) {
            if ((m >> (BPS - 1 - b)) & 1) {
                n1[b] |= vn;
                m1[b] = v < m1[b] ? v : m1[b];
            } else {
                n0[b] |= vn;
                m0[b] = v < m0[b] ? v : m0[b];
            }
        }
    }
#pragma unroll
    for (int b = 0; b < BPS; ++b)
        out[b] = llr_of<T, dm_fast(BPS)>(n0[b] ? (T)NAN : m0[b], n1[b] ? (T)NAN : m1[b], c);   // np.min propagates NaN
}

// sym_llrs_scan_pre (BPSK / QPSK / 8PSK, finite symbols): the scan with the
// unscaled division / square root under one range test per symbol instead of one
// per point (sym_llrs_pairs16): every point's larger |difference| within [2^-80,
// 2^29] (f32) / [2^-800, 2^290] (f64) and nv_fast, for every lane of the wave, or
// false and the caller scans with the per-point tests.  Finite differences below
// 2^29 give finite squares, so np.min's NaN rule never applies; an LLR numerator
// of zero or below the quotient's range takes the compiler's division (its sign of
// zero), per lane.  Measured (profiles/r05/demap_scan/, same planes): 8PSK
// 12.66 -> 11.61 ms, QPSK 5.88 -> 5.70 ms per 1 M codewords.
// The plane kernels take the LLRs' f32 form (llr_from_diff F32OUT = DM_F32OUT):
// same planes, 16QAM 12.62 -> 12.29 ms, 256QAM 12.82 -> 12.30, 8PSK 11.27 -> 11.11 per
// 1 M codewords (profiles/r05/demap_f32out/)
constexpr bool DM_F32OUT = true;
template <typename T, int BPS, bool F32OUT = false, int M = (1 << BPS)>
__device__ __forceinline__ bool sym_llrs_scan_pre(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[BPS]) {
    constexpr bool F32 = sizeof(T) == 4;
    T dx[M], dy[M], lmin = (T)INFINITY, lmax = (T)0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const bool on = M <= 2 || m < c.M;   // a table with fewer points than 2^BPS
        dx[m] = sr - cons[2 * m];
        dy[m] = si - cons[2 * m + 1];
        const T l = fmax(fabs(dx[m]), fabs(dy[m]));
        lmin = on ? fmin(lmin, l) : lmin;
        lmax = on ? fmax(lmax, l) : lmax;
    }
    const bool ok = c.nv_fast && lmin >= (F32 ? (T)0x1p-80f : (T)0x1p-800) && lmax <= (F32 ? (T)0x1p29f : (T)0x1p290);
    if (!__all(ok)) return false;
    T m0[BPS], m1[BPS];
#pragma unroll
    for (int b = 0; b < BPS; ++b) m0[b] = m1[b] = (T)INFINITY;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if (M > 2 && m >= c.M) break;
        const T a = cabs_fin<T, true, true>(dx[m], dy[m]);
        const T v = a * a;                     // np.abs(s - constellation) ** 2
#pragma unroll
        for (int b = 0; b < BPS; ++b) {
            if ((m >> (BPS - 1 - b)) & 1) m1[b] = v < m1[b] ? v : m1[b];
            else m0[b] = v < m0[b] ? v : m0[b];
        }
    }
    const T lo = F32 ? (c.div_f32 ? (T)0x1p-90f : (T)0x1p-149f) : (T)0x1p-900;
#pragma unroll
    for (int b = 0; b < BPS; ++b) {
        const T d = m0[b] - m1[b];
        if (fabs(d) >= lo) out[b] = llr_from_diff<T, true, true, F32OUT>(d, c);
        else out[b] = llr_from_diff<T, false>(d, c);
    }
    return true;
}

// With every lane's symbol finite (the table is), every difference is finite
// and |z| is cabs_fin; BPSK / QPSK / 8PSK (M <= 8, the scan is their only
// path) take that copy when the whole wave qualifies.
template <typename T, int BPS, bool F32OUT = false, int M = (1 << BPS)>
__device__ __forceinline__ void sym_llrs(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[BPS]) {
    if constexpr (M <= 8) {
        if (__all(isfinite(sr) && isfinite(si))) {
            if constexpr (dm_fast(BPS)) {
                if (sym_llrs_scan_pre<T, BPS, F32OUT>(sr, si, cons, c, out)) return;
            }
            sym_llrs_scan<T, BPS, true>(sr, si, cons, c, out);
            return;
        }
    }
    sym_llrs_scan<T, BPS, false>(sr, si, cons, c, out);
}

// 256QAM (K = 4) keeps the previous form of the same search (per-half best and
// second by compare-select, numpy's |z| with its inf / NaN rules): the form
// above compiles to 198-230 VGPRs at K = 4 (2 waves per SIMD, 70.6 -> 100.8 ms
// per 1 M codewords) against 135; at K = 2 / 3 it is 12 % faster.
template <typename T, int BPS>
__device__ __forceinline__ bool sym_llrs_sep_seq(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[BPS]) {
    constexpr int K = BPS / 2, L = 1 << K;
    const T *lev_i = cons + 2 * (1 << BPS), *lev_q = lev_i + L;
    const T inf = (T)INFINITY;
    const T eps = sizeof(T) == 4 ? (T)3.8e-6 : (T)7.2e-15, tau = sizeof(T) == 4 ? (T)1e-30 : (T)1e-290;
    T best[2][K][2], second[2][K][2], all1[2], all2[2];
    int arg[2][K][2], allarg[2];
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        const T s = ax ? si : sr;
        const T *lev = ax ? lev_q : lev_i;
        all1[ax] = all2[ax] = inf;
        allarg[ax] = 0;
#pragma unroll
        for (int b = 0; b < K; ++b)
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                best[ax][b][v] = second[ax][b][v] = inf;
                arg[ax][b][v] = 0;
            }
#pragma unroll
        for (int a = 0; a < L; ++a) {
            const T d = s - lev[a];
            const T d2 = d * d;
            all2[ax] = d2 < all1[ax] ? all1[ax] : (d2 < all2[ax] ? d2 : all2[ax]);
            allarg[ax] = d2 < all1[ax] ? a : allarg[ax];
            all1[ax] = d2 < all1[ax] ? d2 : all1[ax];
#pragma unroll
            for (int b = 0; b < K; ++b) {
                const int v = (a >> (K - 1 - b)) & 1;
                T &b1 = best[ax][b][v], &b2 = second[ax][b][v];
                b2 = d2 < b1 ? b1 : (d2 < b2 ? d2 : b2);
                arg[ax][b][v] = d2 < b1 ? a : arg[ax][b][v];
                b1 = d2 < b1 ? d2 : b1;
            }
        }
    }
    bool ok = all2[0] < inf && all2[1] < inf;   // every value finite (NaN compares false)
#pragma unroll
    for (int ax = 0; ax < 2; ++ax)
#pragma unroll
        for (int b = 0; b < K; ++b)
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const T e = best[ax][b][v] + all1[ax ^ 1];                  // the half's nearest point
                const T tol = eps * e + tau;
                ok = ok && second[ax][b][v] < inf && second[ax][b][v] - best[ax][b][v] > tol &&
                     all2[ax ^ 1] - all1[ax ^ 1] > tol;
            }
    if (!ok) return false;
    // The half holding the overall nearest point has that point as its
    // candidate (same first-minimum rule per axis), so its distance is shared
    // by every bit: BPS + 1 numpy distances instead of 2 * BPS.
    const T an = cabs_fin<T, dm_fast(BPS)>(sr - lev_i[allarg[0]], si - lev_q[allarg[1]]);
    const T dn = an * an;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax)
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const int vn = (allarg[ax] >> (K - 1 - b)) & 1, vo = vn ^ 1;
            const int ia = ax ? allarg[0] : arg[0][b][vo], iq = ax ? arg[1][b][vo] : allarg[1];
            const T a = cabs_fin<T, dm_fast(BPS)>(sr - lev_i[ia], si - lev_q[iq]);
            const T ao = a * a;
            out[ax * K + b] = llr_from_diff<T, dm_fast(BPS)>(vn ? ao - dn : dn - ao, c);   // m[0] - m[1], m[vn] = dn
        }
    return true;
}

// Uniform PAM on each axis with the reference's labelling (sep == 2, detected on
// the host: the 16/64/256QAM tables of sdr_modem.py:142-207 and
// test_sdr_with_coding.py:72-86 put label a at level position gray[a] = a ^ (a >> 1),
// so the label at position p is the inverse Gray code of p -- adjacent levels can
// differ in several label bits).  The same candidates as the searches above, found
// without scanning the 2^K levels: the nearest level position p from
// (s - x_0) / delta, validated by the gap to both neighbours; for label bit b the
// positions with the other bit value nearest to s are the first such position left
// of p and the first right of p (host table nb[b][p] = {left, right}, -1 / L when
// none): every other one lies farther on the same side, since distance grows
// away from s by at least delta^2 per position.  With every decisive gap above the
// tolerance of the largest candidate distance, the argmin of numpy's |s - c|^2 over
// each bit-half is unique and is the candidate, so the LLRs are the full scan's bit
// for bit; anything else (non-finite input, near ties, a wrong position estimate)
// returns false and the caller scans.
__device__ __forceinline__ int gray_inv(int q, int K) {
    int a = q;
    for (int sh = 1; sh < K; ++sh) a ^= q >> sh;
    return a;
}
template <typename T, int BPS, bool F32OUT = false>
__device__ __forceinline__ bool sym_llrs_gray(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[BPS]) {
    constexpr int K = BPS / 2, L = 1 << K;
    if (!(isfinite(sr) && isfinite(si))) return false;
    const T *pos_i = cons + 2 * (1 << BPS) + 2 * L, *pos_q = pos_i + L, *prm = pos_q + L, *nb = prm + 4;
    const T inf = (T)INFINITY;
    const T eps = sizeof(T) == 4 ? (T)3.8e-6 : (T)7.2e-15, tau = sizeof(T) == 4 ? (T)1e-30 : (T)1e-290;
    int p[2], cb[2][K];
    T e0s[2], cds[2][K];   // the nearest level's and the candidates' differences s - level
    T gapmin = inf, dmax = (T)0;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        const T s = ax ? si : sr;
        const T *pos = ax ? pos_q : pos_i;
        const T t = fmin(fmax(rint((s - prm[2 * ax]) * prm[2 * ax + 1]), (T)0), (T)(L - 1));
        const int q = (int)t;
        const T e0 = s - pos[q], d0 = e0 * e0;
        e0s[ax] = e0;
        const T el = s - pos[q > 0 ? q - 1 : q], er = s - pos[q < L - 1 ? q + 1 : q];
        const T dl = q > 0 ? el * el : inf, dr = q < L - 1 ? er * er : inf;
        gapmin = fmin(gapmin, fmin(dl, dr) - d0);
        dmax = fmax(dmax, fmax(d0, fmax(q > 0 ? dl : (T)0, q < L - 1 ? dr : (T)0)));
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const int lc = (int)nb[(b * L + q) * 2], rc = (int)nb[(b * L + q) * 2 + 1];
            const bool lv = lc >= 0, rv = rc < L;
            const T xl = s - pos[lv ? lc : q], xr = s - pos[rv ? rc : q];
            const T dL = lv ? xl * xl : inf, dR = rv ? xr * xr : inf;
            if (lv && rv) gapmin = fmin(gapmin, fabs(dL - dR));
            cb[ax][b] = dL <= dR ? lc : rc;
            cds[ax][b] = dL <= dR ? xl : xr;
            dmax = fmax(dmax, fmax(lv ? dL : (T)0, rv ? dR : (T)0));
        }
        p[ax] = q;
    }
    const T tol = eps * (2 * dmax) + tau;
    if (!(dmax < inf && gapmin > tol)) return false;
    // (a noise variance outside [2^-8, 2^16] declines every symbol to the
    // callers' other searches: the compiler's sequences would hold their
    // registers in this kernel too, a step of occupancy)
    if (!c.nv_fast) return false;
    // the differences the search formed, and one range test per symbol for the
    // unscaled division / square root (sym_llrs_pairs16): every candidate's larger
    // |difference| lies between the axes' nearest differences and sqrt(dmax);
    // outside, or an LLR numerator below the quotient's range, the symbol declines
    // to the full chain
    constexpr bool F32 = sizeof(T) == 4;
    const T l0 = fmax(fabs(e0s[0]), fabs(e0s[1]));
    if (!(l0 >= (F32 ? (T)0x1p-80f : (T)0x1p-800) && dmax <= (F32 ? (T)0x1p58f : (T)0x1p580))) return false;
    const T an = cabs_fin<T, true, true>(e0s[0], e0s[1]);
    const T dq = an * an;
    const T lo = F32 ? (c.div_f32 ? (T)0x1p-90f : (T)0x1p-149f) : (T)0x1p-900;
    T diff[BPS], dlo = inf;
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        const int lab = gray_inv(p[ax], K);
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const int vn = (lab >> (K - 1 - b)) & 1;
            const T a = ax ? cabs_fin<T, true, true>(e0s[0], cds[1][b]) : cabs_fin<T, true, true>(cds[0][b], e0s[1]);
            const T ao = a * a;
            diff[ax * K + b] = vn ? ao - dq : dq - ao;   // m[0] - m[1], m[vn] = dn
            dlo = fmin(dlo, fabs(diff[ax * K + b]));
        }
    }
    if (!(dlo >= lo)) return false;
#pragma unroll
    for (int k = 0; k < BPS; ++k) out[k] = llr_from_diff<T, true, true, F32OUT>(diff[k], c);
    return true;
}

// TDEC_DM_STATS (measurement build): symbols per demap path, read by
// tdec_demap_stats: [0] symbols, [1] taken by the Gray search, [2] by the
// per-axis searches, [3] by the full scan, [4] the table's sep class of the last
// symbol (+1)
#ifndef TDEC_DM_STATS
#define TDEC_DM_STATS 0
#endif
#if TDEC_DM_STATS
__device__ unsigned long long g_dm_stats[8];
__device__ __forceinline__ void dm_count(int path, int sep) {
    atomicAdd(&g_dm_stats[0], 1ull);
    atomicAdd(&g_dm_stats[path], 1ull);
    g_dm_stats[4] = (unsigned long long)(sep + 1);
}
#else
__device__ __forceinline__ void dm_count(int, int) {}
#endif
template <typename T, int BPS, bool F32OUT = false>
__device__ __forceinline__ void demap_sym(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[BPS]) {
    // 64 / 256QAM (measured, 1 M codewords, same planes: 20.2 -> 17.6 ms, 70.3 -> 56.2 ms);
    // 16QAM's 4-level scan is cheaper than the table lookups (14.9 vs 16.0 ms)
    if constexpr (BPS >= 6 && BPS % 2 == 0) {
        if (c.sep == 2 && sym_llrs_gray<T, BPS, F32OUT>(sr, si, cons, c, out)) return dm_count(1, c.sep);
    }
    if constexpr (BPS >= 8 && BPS % 2 == 0) {
        if (c.sep && sym_llrs_sep_seq<T, BPS>(sr, si, cons, c, out)) return dm_count(2, c.sep);
    } else if constexpr (BPS >= 4 && BPS % 2 == 0) {
        if (c.sep && sym_llrs_sep<T, BPS, F32OUT>(sr, si, cons, c, out)) return dm_count(2, c.sep);
    }
    sym_llrs<T, BPS, F32OUT>(sr, si, cons, c, out);
    dm_count(3, c.sep);
}

// The table (and a separable table's axis levels) into LDS.
template <typename T, int BPS> __device__ __forceinline__ void load_table(T *cons, const T *cons_g, const DemapCfg &c) {
    constexpr int L = 1 << (BPS / 2);
    const int n = 2 * c.M + (c.sep ? 2 * L : 0) + (c.sep == 2 ? 2 * L + 4 + 2 * (BPS / 2) * L : 0);
    for (int i = threadIdx.x; i < n; i += BLOCK) cons[i] = cons_g[i];
}

template <typename T, typename S, int BPS, int ROWNV = 0>
__global__ __launch_bounds__(BLOCK) void k_demap(const S *syms, long n_sym, const T *cons_g, DemapCfg c, double *llr,
                                                RowNv<ROWNV> rn = {}) {
    __shared__ T cons[DM_TAB];
    load_table<T, BPS>(cons, cons_g, c);
    __syncthreads();
    const long s = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_sym) return;
    double v[BPS];
    demap_sym<T, BPS>((T)syms[2 * s], (T)syms[2 * s + 1], cons, cfg_at(c, rn, s), v);
#pragma unroll
    for (int b = 0; b < BPS; ++b) llr[s * BPS + b] = v[b];
}

// Fused demap -> f32 -> de-puncture planes (the bench path).
// One item = one 64-codeword tile x DM_KC trellis steps (one block per item).
// Phase 1: the block's threads demap every symbol covering the LLR range of those
// steps (couples consume LLRs in order, so the range is contiguous) into an LDS
// tile, decoder sign, rounded to f32 as decode() does (:466).  Phase 2: each
// thread assembles whole plane entries X[k] = {A, B, W1, Y1} (float4), Z[k] =
// {W2, Y2} (float2) and stores them coalesced; punctured or missing LLRs are 0.0
// (:469-474; the harness pads to n_coded, test_sdr_with_coding.py:474-478).
// src[c*N + k] = LLR index of plane component c (X.xyzw, -, -, Z.xy) or -1;
// off[k] = first LLR index of couple k (off[N] = n_llr).
// Split tables (round 4, square 16 / 64 / 256QAM): k_demap_planes runs only the
// fast exact search (the Gray positions for 64 / 256QAM, the per-axis search for
// 16QAM) and appends the symbols it declines (near ties, non-finite input, a
// non-separable table: 0.02-0.08 % of them at 2 dB) to a list in HBM; k_demap_fix
// then gives those the rest of demap_sym's chain and overwrites their plane
// entries.  The fallbacks' registers (256QAM: 148 VGPRs and 311 SGPR spills with
// them inline, three waves per SIMD) are then not the main kernel's.  A tile whose
// declines overflow the list is flagged and k_demap_fix redoes all of its symbols.
// Same planes: every path returns the scan's LLRs.  (The fallback in a second loop
// of the same kernel kept the registers and was 2.3x slower on 256QAM,
// profiles/r04e/ab_demap_*; a persistent grid, one wave per 16 codewords, and the
// other forms in the DESIGN.md appendix measured slower.)
// KC: couples per block (its LDS tile [64][6 * KC + 2 * BPS + 1] f32 bounds the
// blocks per CU: 16 -> 27-29 KB, five).  QPSK's kernel is LDS-bound at five blocks
// per CU and its work per block small: 12 couples measured faster (5.47 vs 5.82 ms
// per 1 M N = 212 codewords); 16QAM slower with 12 or 8 (13.45 / 13.41 vs 12.75 ms,
// profiles/r05/demap_kc/).
constexpr int DM_KC = 16;                  // couples per block
constexpr int DM_MAXL = DM_KC * 6;         // max LLRs per chunk (6 per couple at rate 1/3)
__host__ __device__ constexpr int dm_kc(int bps) { return bps == 2 ? 12 : DM_KC; }
__host__ __device__ constexpr bool dm_split(int bps) { return bps >= 4 && bps % 2 == 0; }

// The decline list of k_demap_planes (split tables): entries {codeword, symbol},
// the entry count, and per-tile overflow flags.
constexpr unsigned DM_DECL_CAP = 1u << 21;   // entries (16 MiB): 4x the declines of 1 M 256QAM codewords at 2 dB
// A table takes the split path when its fast search can accept its symbols: the
// Gray search (64 / 256QAM) needs sep == 2, 16QAM's per-axis search sep >= 1;
// any other table would decline every symbol.
__host__ __device__ constexpr bool dm_split_table(int bps, int sep) {
    return dm_split(bps) && (bps >= 6 ? sep == 2 : sep >= 1);
}
struct DemapDecl {
    int2 *list;
    unsigned *count;
    unsigned char *ovf;
    unsigned cap;
};

// the fast exact search of a split table; false: declined
template <typename T, int BPS, bool F32OUT = false>
__device__ __forceinline__ bool demap_fast(T sr, T si, const T *cons, const DemapCfg &c, double (&out)[BPS]) {
    if constexpr (BPS >= 6) return c.sep == 2 && sym_llrs_gray<T, BPS, F32OUT>(sr, si, cons, c, out);
    else return c.sep && sym_llrs_sep<T, BPS, F32OUT>(sr, si, cons, c, out);
}

// ROWNV: neighbouring threads of an item belong to different rows of the tile, so each
// symbol's configuration comes from its own value (cfg_at; DESIGN.md §10 has the tile's 64
// values staged in LDS measured against it).
template <typename T, int BPS, bool SPLIT = false, int ROWNV = 0>
__global__ __launch_bounds__(BLOCK) void k_demap_planes(int B, int N, int S, const float *syms, const T *cons_g,
                                                       DemapCfg c, const int *__restrict__ src,
                                                       const int *__restrict__ off, long n_avail, float *planes,
                                                       long n_items, DemapDecl dd, RowNv<ROWNV> rn = {}) {
    __shared__ T cons[DM_TAB];
    // couples per item, LDS row stride (odd); the tile by label bit (column b * ns +
    // symbol: the 64 lanes of a phase-1 store hit 64 banks, 1.5-4 % faster on every
    // table, profiles/r05/demap_planar/) with room for the item's straddling symbols
    constexpr int KC = dm_kc(BPS), LD = 6 * KC + 2 * BPS + 1;
    __shared__ float L[WAVE * LD];
    static_assert(!SPLIT || dm_split(BPS), "split only for square 16 / 64 / 256QAM");
    const int me = (int)threadIdx.x & (WAVE - 1);
    load_table<T, BPS>(cons, cons_g, c);
    const int chunks = (N + KC - 1) / KC;
    __syncthreads();
    for (long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const long tile = item / chunks;
        const int k0 = (int)(item % chunks) * KC;
        const int k1 = min(N, k0 + KC);
        const long j0 = off[k0], j1 = off[k1];
        const long s0 = j0 / BPS, s1 = (j1 + BPS - 1) / BPS;        // symbols covering [j0, j1)
        const int ns = (int)(s1 - s0);
        // item t = (lane, si), consecutive threads: consecutive symbols; the
        // quotient and remainder of t by ns advance by those of BLOCK each step
        const int T0 = (int)threadIdx.x;
        const int dq = BLOCK / ns, dr = BLOCK - dq * ns;
        int lane = T0 / ns, si = T0 - lane * ns;
        const int nt = WAVE * ns;
        // the symbol of item t (lane ln, symbol sx), zero past the batch / the item's end
        auto sym_at = [&](int t, int ln, int sx) -> float2 {
            const long cw = tile * WAVE + ln, s = s0 + sx;
            return t < nt && cw < B && s < S ? *reinterpret_cast<const float2 *>(syms + 2 * (cw * S + s))
                                             : make_float2(0.0f, 0.0f);
        };
        // the next item's symbol is loaded before this one is demapped (8PSK / 16QAM:
        // measured faster; QPSK and 64 / 256QAM slower)
        constexpr bool PF = BPS == 3 || BPS == 4;
        float2 zn = PF ? sym_at(T0, lane, si) : make_float2(0.0f, 0.0f);
        for (int t = T0; t < nt; t += BLOCK) {
            const int ln = lane, sx = si;
            lane += dq;
            si += dr;
            if (si >= ns) {
                si -= ns;
                ++lane;
            }
            const float2 zc = PF ? zn : sym_at(t, ln, sx);
            if (PF) zn = sym_at(t + BLOCK, lane, si);
            const long cw = tile * WAVE + ln;
            const long s = s0 + sx;
            const bool live = cw < B && s < S;
            double v[BPS];
            if constexpr (SPLIT) {
                bool dec = false;
                if (live) dec = !demap_fast<T, BPS, DM_F32OUT>((T)zc.x, (T)zc.y, cons, cfg_at(c, rn, cw, s), v);
                // declined symbols go to the list for k_demap_fix (which rewrites their
                // plane entries): one atomic per wave, entries by lane rank
                const unsigned long long m = __ballot(dec);
                if (m) {
                    const int leader = __ffsll((long long)m) - 1;
                    unsigned base = 0;
                    if (me == leader) base = atomicAdd(dd.count, (unsigned)__popcll(m));
                    base = __shfl(base, leader);
                    if (dec) {
                        const unsigned e = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                                           __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                        if (e < dd.cap) dd.list[e] = make_int2((int)cw, (int)s);
                        else dd.ovf[tile] = 1;
                    }
                }
                if (!live || dec) continue;
            } else {
                if (!live) continue;
                demap_sym<T, BPS, DM_F32OUT>((T)zc.x, (T)zc.y, cons, cfg_at(c, rn, cw, s), v);
            }
#pragma unroll
            for (int b = 0; b < BPS; ++b) L[ln * LD + b * ns + sx] = (float)v[b];
        }
        float *base = planes + tile * tile_floats(N);
        __syncthreads();
        for (int t = threadIdx.x; t < WAVE * (k1 - k0) * 2; t += BLOCK) {
            const int lane = t & (WAVE - 1);
            const int q = __builtin_amdgcn_readfirstlane(t >> 6);   // (step, half): wave-uniform, so src[] is read by scalar loads
            const int k = k0 + q / 2, half = q & 1;
            const long cw = tile * WAVE + lane;
            const int nc = half ? 2 : 4;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                if (cc >= nc) break;
                const int j = src[(long)(half ? 6 + cc : cc) * N + k];
                const int col = j >= 0 ? (j % BPS) * ns + (int)(j / BPS - s0) : 0;
                v[cc] = (j >= 0 && j < n_avail && cw < B) ? L[lane * LD + col] : 0.0f;
            }
            if (half == 0) reinterpret_cast<float4 *>(base)[(long)k * WAVE + lane] = make_float4(v[0], v[1], v[2], v[3]);
            else reinterpret_cast<float2 *>(base + (long)N * WAVE * 4)[(long)k * WAVE + lane] = make_float2(v[0], v[1]);
        }
        __syncthreads();   // L is rewritten by the next item: its reads done everywhere
    }
}

// The declined symbols of k_demap_planes (split tables): demap_sym's whole chain,
// each LLR into its plane entry (dst[j] = c * N + k for the component c of couple
// k that LLR j feeds, -1: none), then every symbol of an overflowed tile.
template <typename T, int BPS>
__device__ __forceinline__ void dm_fix_symbol(long cw, long s, int N, int S, const float *syms, const T *cons,
                                              const DemapCfg &c, const int *dst, long n_avail, float *planes) {
    const float2 z = *reinterpret_cast<const float2 *>(syms + 2 * (cw * S + s));
    double v[BPS];
    demap_sym<T, BPS, DM_F32OUT>((T)z.x, (T)z.y, cons, c, v);
    float *base = planes + (cw / WAVE) * tile_floats(N);
    const int lane = (int)(cw & (WAVE - 1));
#pragma unroll
    for (int b = 0; b < BPS; ++b) {
        const long j = s * BPS + b;
        if (j >= n_avail) break;
        const int d = dst[j];
        if (d < 0) continue;
        const int cc = d / N, k = d - cc * N;
        if (cc < 4) base[((long)k * WAVE + lane) * 4 + cc] = (float)v[b];
        else base[(long)N * WAVE * 4 + ((long)k * WAVE + lane) * 2 + (cc - 6)] = (float)v[b];
    }
}
template <typename T, int BPS, int ROWNV = 0>
__global__ __launch_bounds__(BLOCK) void k_demap_fix(int B, int N, int S, const float *syms, const T *cons_g,
                                                    DemapCfg c, const int *__restrict__ dst, long n_avail,
                                                    float *planes, DemapDecl dd, long n_tiles, RowNv<ROWNV> rn = {}) {
    __shared__ T cons[DM_TAB];
    load_table<T, BPS>(cons, cons_g, c);
    __syncthreads();
    const unsigned n = min(*dd.count, dd.cap);
    for (unsigned i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const int2 e = dd.list[i];
        if (dd.ovf[e.x / WAVE]) continue;   // redone below
        dm_fix_symbol<T, BPS>(e.x, e.y, N, S, syms, cons, cfg_at(c, rn, e.x, e.y), dst, n_avail, planes);
    }
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        if (!dd.ovf[t]) continue;
        for (long i = threadIdx.x; i < (long)WAVE * S; i += BLOCK) {
            const long cw = t * WAVE + i / S;
            if (cw < B) dm_fix_symbol<T, BPS>(cw, i % S, N, S, syms, cons, cfg_at(c, rn, cw, i % S), dst, n_avail, planes);
        }
    }
}

// ---- log-MAP (exact log-sum) soft demapper (build-defined) -------------
//   d_i = |s - c_i|^2,  L_b,v = log sum_{i : bit_b(i) = v} exp(-d_i / nv),
//   llr_b = sign * clip(L_b,1 - L_b,0, -30, +30)
// with the max-log path's nv floor, clip and sign; the max-log demapper is this
// formula's max-log approximation.  Evaluated in base 2: x_i = d_i * scale with
// scale = 1 / (nv ln 2) (one host division per launch), every term against the
// smallest x_i (the largest term is exactly 1, no cut-off), and
// llr = ln 2 * (log2 S_1 - log2 S_0): the shift cancels.  f32 arithmetic uses
// v_exp_f32 / v_log_f32 (hw_exp2 / hw_log2, quarter-rate VALU), f64 arithmetic the
// library's exp2 / log2.  Tolerance-defined (DESIGN.md §9 has the error model and the
// measured constant), not pinned to numpy: no decline list and no fix-up kernel.
// A half no point of the table carries, or one whose terms all underflow, gives
// log2 0 = -inf and so +-30.  NaN or infinite symbols give NaN (inf - inf).
template <typename T> __device__ __forceinline__ T lm_exp2(T x);
template <> __device__ __forceinline__ float lm_exp2<float>(float x) { return hw_exp2(x); }
template <> __device__ __forceinline__ double lm_exp2<double>(double x) { return exp2(x); }
template <typename T> __device__ __forceinline__ T lm_log2(T x);
template <> __device__ __forceinline__ float lm_log2<float>(float x) { return hw_log2(x); }
template <> __device__ __forceinline__ double lm_log2<double>(double x) { return log2(x); }
template <typename T> __device__ __forceinline__ T lm_min(T a, T b);   // minNum: a NaN operand is dropped
template <> __device__ __forceinline__ float lm_min<float>(float a, float b) { return __builtin_fminf(a, b); }
template <> __device__ __forceinline__ double lm_min<double>(double a, double b) { return __builtin_fmin(a, b); }

template <typename T> __device__ __forceinline__ double lm_llr(T s0, T s1, const DemapCfg &c) {
    T v = (lm_log2<T>(s1) - lm_log2<T>(s0)) * (T)0.693147180559945309417;
    if (v == v) v = v < (T)-30 ? (T)-30 : (v > (T)30 ? (T)30 : v);
    return (double)(c.sign < 0 ? -v : v);
}

// The two sums of every label bit (MSB first) over the 2^K terms e[label]: the
// halves of e are the leading bit's sums; folding one half onto the other
// marginalises that bit and leaves the same problem with K - 1 bits
// (36 additions for K = 4 instead of 56).  e is consumed.
template <typename T, int K> __device__ __forceinline__ void lm_bit_sums(T (&e)[1 << K], T (&s0)[K], T (&s1)[K]) {
#pragma unroll
    for (int b = 0; b < K; ++b) {
        const int h = 1 << (K - 1 - b);
        T a0 = e[0], a1 = e[h];
#pragma unroll
        for (int j = 1; j < h; ++j) {
            a0 += e[j];
            a1 += e[h + j];
        }
        s0[b] = a0;
        s1[b] = a1;
#pragma unroll
        for (int j = 0; j < h; ++j) e[j] += e[h + j];
    }
}

// Separable square QAM (DemapCfg::sep, point (a, q) = levI[a] + j levQ[q]):
// exp(-d / nv) = exp(-dI / nv) exp(-dQ / nv), so a sum over a half of the grid that
// an I bit selects is (sum over that bit's half of the I levels) x (sum over all Q
// levels), and the second factor cancels in L_b,1 - L_b,0: each axis' K bits need
// that axis' 2^K exponentials only (256QAM: 32 + 16 logarithms per symbol, against
// 256 + 16 for the scan).  A non-finite coordinate must reach the other axis'
// bits too (every d_i is NaN or inf then): it is added to both axes' shifts.
template <typename T, int BPS>
__device__ __forceinline__ void lm_sym_sep(T sr, T si, const T *cons, const DemapCfg &c, T scale, double (&out)[BPS]) {
    constexpr int K = BPS / 2, L = 1 << K;
    const T *lev = cons + 2 * c.M;
    const T poison = (sr - sr) + (si - si);   // 0, or NaN for a NaN / infinite symbol
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        const T s = ax ? si : sr;
        T x[L], e[L], xm = (T)INFINITY;
#pragma unroll
        for (int a = 0; a < L; ++a) {
            const T dz = s - lev[ax * L + a];   // LDS, the same address in every lane: a broadcast read
            x[a] = dz * dz * scale;
            xm = lm_min<T>(xm, x[a]);
        }
        xm += poison;
#pragma unroll
        for (int a = 0; a < L; ++a) e[a] = lm_exp2<T>(xm - x[a]);
        T s0[K], s1[K];
        lm_bit_sums<T, K>(e, s0, s1);
#pragma unroll
        for (int b = 0; b < K; ++b) out[ax * K + b] = lm_llr<T>(s0[b], s1[b], c);
    }
}

// Any other table: two passes over its M points (the smallest x, then the terms),
// so no distance array is kept; up to 16 points the passes unroll and share the x.
template <typename T, int BPS, int M = (1 << BPS), int UNROLL = (M <= 16 ? M : 8)>
__device__ __forceinline__ void lm_sym_scan(T sr, T si, const T *cons, const DemapCfg &c, T scale, double (&out)[BPS]) {
    auto x_at = [&](int m) -> T {
        const T dx = sr - cons[2 * m], dy = si - cons[2 * m + 1];
        return (dx * dx + dy * dy) * scale;
    };
    T xm = (T)INFINITY;   // stays inf for a NaN symbol: inf - NaN below
#pragma unroll UNROLL
    for (int m = 0; m < M; ++m) {
        if (M > 2 && m >= c.M) break;
        xm = lm_min<T>(xm, x_at(m));
    }
    T s0[BPS], s1[BPS];
#pragma unroll
    for (int b = 0; b < BPS; ++b) s0[b] = s1[b] = (T)0;
#pragma unroll UNROLL
    for (int m = 0; m < M; ++m) {
        if (M > 2 && m >= c.M) break;
        const T e = lm_exp2<T>(xm - x_at(m));
#pragma unroll
        for (int b = 0; b < BPS; ++b) {
            if ((m >> (BPS - 1 - b)) & 1) s1[b] += e;
            else s0[b] += e;
        }
    }
#pragma unroll
    for (int b = 0; b < BPS; ++b) out[b] = lm_llr<T>(s0[b], s1[b], c);
}

template <typename T, int BPS>
__device__ __forceinline__ void demap_lm_sym(T sr, T si, const T *cons, const DemapCfg &c, T scale, double (&out)[BPS]) {
    if constexpr (BPS >= 4 && BPS % 2 == 0) {
        if (c.sep) return lm_sym_sep<T, BPS>(sr, si, cons, c, scale, out);
    }
    lm_sym_scan<T, BPS>(sr, si, cons, c, scale, out);
}

// k_demap's launch shape: one symbol per thread, f64 LLRs
template <typename T, typename S, int BPS, int ROWNV = 0>
__global__ __launch_bounds__(BLOCK) void k_demap_lm(const S *syms, long n_sym, const T *cons_g, DemapCfg c, double scale,
                                                   double *llr, RowNv<ROWNV> rn = {}) {
    __shared__ T cons[DM_TAB];
    load_table<T, BPS>(cons, cons_g, c);
    __syncthreads();
    const long s = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_sym) return;
    double v[BPS];
    const DemapCfg &rc = cfg_at(c, rn, s);
    demap_lm_sym<T, BPS>((T)syms[2 * s], (T)syms[2 * s + 1], cons, rc, lm_scale_at(rc, rn, (T)scale), v);
#pragma unroll
    for (int b = 0; b < BPS; ++b) llr[s * BPS + b] = v[b];
}

// k_demap_planes' items, LDS tile and plane layout (its phase 2 verbatim, so
// tdec_decode_planes_dev consumes these planes unchanged) around demap_lm_sym;
// no split and no prefetch: the symbol's work is the transcendentals.
template <typename T, int BPS, int ROWNV = 0>
__global__ __launch_bounds__(BLOCK) void k_demap_planes_lm(int B, int N, int S, const float *syms, const T *cons_g,
                                                          DemapCfg c, double scale, const int *__restrict__ src,
                                                          const int *__restrict__ off, long n_avail, float *planes,
                                                          long n_items, RowNv<ROWNV> rn = {}) {
    __shared__ T cons[DM_TAB];
    constexpr int KC = dm_kc(BPS), LD = 6 * KC + 2 * BPS + 1;
    __shared__ float L[WAVE * LD];
    load_table<T, BPS>(cons, cons_g, c);
    const int chunks = (N + KC - 1) / KC;
    const T sc = (T)scale;
    __syncthreads();
    for (long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const long tile = item / chunks;
        const int k0 = (int)(item % chunks) * KC;
        const int k1 = min(N, k0 + KC);
        const long j0 = off[k0], j1 = off[k1];
        const long s0 = j0 / BPS, s1 = (j1 + BPS - 1) / BPS;        // symbols covering [j0, j1)
        const int ns = (int)(s1 - s0);
        for (int t = threadIdx.x; t < WAVE * ns; t += BLOCK) {      // consecutive threads: consecutive symbols
            const int ln = t / ns, sx = t - ln * ns;
            const long cw = tile * WAVE + ln, s = s0 + sx;
            if (cw >= B || s >= S) continue;
            const float2 z = *reinterpret_cast<const float2 *>(syms + 2 * (cw * S + s));
            double v[BPS];
            const DemapCfg &rc = cfg_at(c, rn, cw, s);
            demap_lm_sym<T, BPS>((T)z.x, (T)z.y, cons, rc, lm_scale_at(rc, rn, sc), v);
#pragma unroll
            for (int b = 0; b < BPS; ++b) L[ln * LD + b * ns + sx] = (float)v[b];
        }
        float *base = planes + tile * tile_floats(N);
        __syncthreads();
        for (int t = threadIdx.x; t < WAVE * (k1 - k0) * 2; t += BLOCK) {
            const int lane = t & (WAVE - 1);
            const int q = __builtin_amdgcn_readfirstlane(t >> 6);   // (step, half): wave-uniform
            const int k = k0 + q / 2, half = q & 1;
            const long cw = tile * WAVE + lane;
            const int nc = half ? 2 : 4;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                if (cc >= nc) break;
                const int j = src[(long)(half ? 6 + cc : cc) * N + k];
                const int col = j >= 0 ? (j % BPS) * ns + (int)(j / BPS - s0) : 0;
                v[cc] = (j >= 0 && j < n_avail && cw < B) ? L[lane * LD + col] : 0.0f;
            }
            if (half == 0) reinterpret_cast<float4 *>(base)[(long)k * WAVE + lane] = make_float4(v[0], v[1], v[2], v[3]);
            else reinterpret_cast<float2 *>(base + (long)N * WAVE * 4)[(long)k * WAVE + lane] = make_float2(v[0], v[1]);
        }
        __syncthreads();   // L is rewritten by the next item: its reads done everywhere
    }
}

// ---- per-row noise variance estimate (build-defined) -------------------
// The decision-directed estimate of test_sdr_with_coding.py:459-467, one value per
// row of [B][S] complex64 symbols:
//   e_s = min_m (dx*dx + dy*dy), dx / dy the f64 differences of the f32 symbol and
//   table point m (the first minimum in label order: the hard decision re-mapped),
//   nv[r] = max_py(sum_s e_s / S, floor),  max_py(a, b) = (b > a) ? b : a
// (a NaN mean stays NaN, Python's max(nv, 0.02)).  A NaN or infinite symbol makes its
// e_s, and so its row's estimate, NaN.  One block per row; the f64 sum has a fixed
// order (thread t adds symbols t, t + BLOCK, ... in turn, the 64 partial sums of a wave
// fold by an xor butterfly, thread 0 adds the four wave sums in order), so a row's
// value depends on neither B nor the grid.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_noise_var(const float *syms, int S, const T *cons_g, int M, double floor_nv,
                                                    double *nv) {
    __shared__ double cons[2 * 256];
    __shared__ double part[BLOCK / WAVE];
    for (int i = threadIdx.x; i < 2 * M; i += BLOCK) cons[i] = (double)cons_g[i];
    __syncthreads();
    const float *row = syms + 2 * (long)blockIdx.x * S;
    double acc = 0.0;
    for (int s = threadIdx.x; s < S; s += BLOCK) {
        const float2 z = *reinterpret_cast<const float2 *>(row + 2 * s);
        const double sr = (double)z.x, si = (double)z.y;
        double e = INFINITY;
        for (int m = 0; m < M; ++m) {
            const double dx = sr - cons[2 * m], dy = si - cons[2 * m + 1];
            const double d = dx * dx + dy * dy;
            if (d < e) e = d;
        }
        acc += e + ((sr - sr) + (si - si));   // + 0, or NaN for a NaN / infinite symbol
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = part[0];
#pragma unroll
        for (int w = 1; w < BLOCK / WAVE; ++w) sum += part[w];
        const double mean = sum / (double)S;
        nv[blockIdx.x] = (floor_nv > mean) ? floor_nv : mean;
    }
}

// ---- flat-fading equaliser (build-defined) -------------------------------
// y = h x + n with known h: z = y / h and the noise variance of z, nv / |h|^2, for each
// symbol of [B][S] complex64 rows; symbol s of row r uses h[r][s / coh] of
// [B][ceil(S / coh)] gains.  All in f64, no contraction:
//   g = hr*hr + hi*hi   (the products of f32 values are exact in f64: one rounding)
//   z = ((float)((yr*hr + yi*hi) / g), (float)((yi*hr - yr*hi) / g)),  nv_sym = nv_r / g
// (no floor here: the demapper floors).  g == 0 or not finite: an erasure, z = 0 and
// nv_sym = +inf, which the demappers turn into all-zero LLRs.  NVROWS: nv_r = nvs[r] (a
// device vector), else the launch's nv.  One thread per symbol; with VEC one thread per
// two consecutive symbols of the flat [B * S] array (which may lie in two rows), so y is
// read and z and nv_sym are written 16 bytes at a time (the host checks the alignment).
struct EqOut {
    float zr, zi;
    double nv;
};
__device__ __forceinline__ EqOut eq_symbol(float2 y, float2 h, double nv) {
    const double hr = (double)h.x, hi = (double)h.y, yr = (double)y.x, yi = (double)y.y;
    const double g = hr * hr + hi * hi;
    if (g == 0.0 || !(fabs(g) < INFINITY)) return EqOut{0.0f, 0.0f, (double)INFINITY};
    return EqOut{(float)((yr * hr + yi * hi) / g), (float)((yi * hr - yr * hi) / g), nv / g};
}
template <bool NVROWS, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_equalize(const float2 *y, const float2 *h, long n_sym, int S, int coh, int nh,
                                                   double nv, const double *nvs, float2 *z, double *nv_sym) {
    const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
    auto one = [&](long i, float2 yi) -> EqOut {   // i < n_sym
        const long r = i / S;
        const int s = (int)(i - r * S);
        return eq_symbol(yi, h[r * nh + s / coh], NVROWS ? nvs[r] : nv);
    };
    if constexpr (VEC) {
        const long i = 2 * t;
        if (i + 1 < n_sym) {
            const float4 yy = reinterpret_cast<const float4 *>(y)[t];
            const EqOut a = one(i, make_float2(yy.x, yy.y)), b = one(i + 1, make_float2(yy.z, yy.w));
            reinterpret_cast<float4 *>(z)[t] = make_float4(a.zr, a.zi, b.zr, b.zi);
            reinterpret_cast<double2 *>(nv_sym)[t] = make_double2(a.nv, b.nv);
        } else if (i < n_sym) {   // the last symbol of an odd count
            const EqOut a = one(i, y[i]);
            z[i] = make_float2(a.zr, a.zi);
            nv_sym[i] = a.nv;
        }
    } else {
        if (t >= n_sym) return;
        const EqOut a = one(t, y[t]);
        z[t] = make_float2(a.zr, a.zi);
        nv_sym[t] = a.nv;
    }
}

// ---- receive diversity: maximal-ratio combiner (build-defined) ------------
// R copies of a burst, y [B][R][S] complex64 through the gains h [B][R][ceil(S / coh)], into
// what k_equalize writes for one: z [B][S] and nv_sym [B][S].  All in f64, no contraction,
// the branches in the order r = 0 .. R-1.  Per branch
//   g = hr*hr + hi*hi,  a = yr*hr + yi*hi,  b = yi*hr - yr*hi
// and a branch whose g is zero or not finite is skipped.  NV 0 / 1, a common noise variance
// (the launch's nv / nvs[row]): G, A, Bm are the sums of g, a, b over the live branches,
//   z = ((float)(A / G), (float)(Bm / G)),  nv_sym = nv_b / G.
// NV 2, nvs[row][r] per branch: the summed terms are g / nv_br, a / nv_br, b / nv_br,
//   z likewise,  nv_sym = 1.0 / G.
// Each sum starts from the first live branch's term, not from 0.0 (a -0.0 numerator keeps
// its sign), so R = 1 with a common noise is eq_symbol bit for bit.  No live branch, or a
// G that came out zero or infinite: an erasure, z = 0 and nv_sym = +inf.  A NaN G (a NaN
// nv_br, §10's convention) stays NaN in z and nv_sym.
// One thread per symbol; with VEC one thread per two consecutive symbols of a row (S is
// even, so a pair never straddles rows, and every base is 16-byte aligned: the host checks
// both), each branch's y read and z and nv_sym written 16 bytes at a time.  Consecutive
// lanes take consecutive s, so every branch's loads are coalesced; a symbol's R branches
// lie S apart.
struct MrcSum {
    double G, A, Bm;
    bool live;
};
template <int NV>
__device__ __forceinline__ void mrc_add(MrcSum &m, float2 y, float2 h, double nv_br) {
    const double hr = (double)h.x, hi = (double)h.y, yr = (double)y.x, yi = (double)y.y;
    const double g = hr * hr + hi * hi;
    if (g == 0.0 || !(fabs(g) < INFINITY)) return;   // a dead branch vouches for nothing
    double gg = g, a = yr * hr + yi * hi, b = yi * hr - yr * hi;
    if constexpr (NV == 2) {
        gg = g / nv_br;
        a = a / nv_br;
        b = b / nv_br;
    }
    if (m.live) {
        m.G += gg;
        m.A += a;
        m.Bm += b;
    } else {
        m = MrcSum{gg, a, b, true};
    }
}
template <int NV>
__device__ __forceinline__ EqOut mrc_out(const MrcSum &m, double nv) {
    if (!m.live || m.G == 0.0 || fabs(m.G) == (double)INFINITY) return EqOut{0.0f, 0.0f, (double)INFINITY};
    return EqOut{(float)(m.A / m.G), (float)(m.Bm / m.G), (NV == 2 ? 1.0 : nv) / m.G};
}
template <int NV, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_combine(const float2 *y, const float2 *h, long n_sym, int R, int S, int coh,
                                                  int nh, double nv, const double *nvs, float2 *z, double *nv_sym) {
    const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
    const long i = VEC ? 2 * t : t;                  // VEC: n_sym is even
    if (i >= n_sym) return;
    const long row = i / S;
    const int s = (int)(i - row * S);
    const float2 *yb = y + row * R * S + s, *hb = h + row * R * nh;
    const double nv_c = NV == 1 ? nvs[row] : nv;
    const int j0 = s / coh, j1 = VEC ? (s + 1) / coh : 0;
    MrcSum m0{}, m1{};
    for (int r = 0; r < R; ++r) {
        const double nv_br = NV == 2 ? nvs[row * R + r] : 0.0;
        if constexpr (VEC) {
            const float4 yy = *reinterpret_cast<const float4 *>(yb + (long)r * S);
            mrc_add<NV>(m0, make_float2(yy.x, yy.y), hb[r * nh + j0], nv_br);
            mrc_add<NV>(m1, make_float2(yy.z, yy.w), hb[r * nh + j1], nv_br);
        } else {
            mrc_add<NV>(m0, yb[(long)r * S], hb[r * nh + j0], nv_br);
        }
    }
    const EqOut a = mrc_out<NV>(m0, nv_c);
    if constexpr (VEC) {
        const EqOut b = mrc_out<NV>(m1, nv_c);
        reinterpret_cast<float4 *>(z)[t] = make_float4(a.zr, a.zi, b.zr, b.zi);
        reinterpret_cast<double2 *>(nv_sym)[t] = make_double2(a.nv, b.nv);
    } else {
        z[i] = make_float2(a.zr, a.zi);
        nv_sym[i] = a.nv;
    }
}

// ---- fused demap + decode ------------------------------------------------------------
// Each persistent decoder wave demaps its next 64-codeword tile itself (the same
// operations as k_demap_planes, so the planes are bit-identical) into a plane
// buffer of its own, then decodes it.  The demap is VALU-bound and the decoder
// HBM-bound, so inside one launch the demap's arithmetic runs while the other
// waves stream the decoder's planes (a separate k_demap_planes launch serialises
// them), and the plane buffer is sized per resident wave, not per codeword.
constexpr int DF_KC = 8;                   // couples per LDS chunk
constexpr int DF_LD = DF_KC * 6 + 1;       // odd row stride

struct FusedDemapArgs {
    const float *syms;                     // [B][S] complex64
    int S;
    long n_avail;                          // LLRs the symbols provide (<= the de-puncture walk)
    const int *src, *off;                  // de-puncture map (tdec_create)
    float *planes_w;                       // [n_waves][2] x tile_floats(N): the wave's current and next tile
    DemapCfg c;
    const void *cons_g;                    // device table (T)
};

template <typename T, int BPS> struct DemapPro {
    FusedDemapArgs a;                       // by value: SGPRs, no address of a kernel argument
    int B;
    const T *cons;                          // LDS copy
    float *L;                               // this wave's LDS chunk [64][DF_LD]
    __device__ __forceinline__ const float *tile_planes(int /*tile*/, int wave, int N, int buf) const {
        return a.planes_w + (2L * wave + buf) * tile_floats(N);
    }
    // chunks [piece/npieces, (piece+1)/npieces) of the tile's DF_KC-couple chunks
    __device__ __forceinline__ void fill(int tile, int wave, int N, int buf, int piece, int npieces) const {
        const int lane = threadIdx.x & (WAVE - 1);
        float *pl = a.planes_w + (2L * wave + buf) * tile_floats(N);
        float4 *X = reinterpret_cast<float4 *>(pl);
        float2 *Z = reinterpret_cast<float2 *>(pl + (long)N * WAVE * 4);
        const int S = a.S;
        const int nch = (N + DF_KC - 1) / DF_KC;
        const int c0 = piece * nch / npieces, c1 = (piece + 1) * nch / npieces;
        for (int ch = c0; ch < c1; ++ch) {
            const int k0 = ch * DF_KC, k1 = min(N, k0 + DF_KC);
            const long j0 = a.off[k0], j1 = a.off[k1];
            const long s0 = j0 / BPS, s1 = (j1 + BPS - 1) / BPS;   // symbols covering [j0, j1)
            const int ns = (int)(s1 - s0);
            for (int t = lane; t < WAVE * ns; t += WAVE) {
                const int l = t / ns, si = t - l * ns;              // consecutive lanes: consecutive symbols
                const long cw = (long)tile * WAVE + l;
                const long sy = s0 + si;
                if (cw >= B || sy >= S) continue;
                const float2 z = *reinterpret_cast<const float2 *>(a.syms + 2 * (cw * S + sy));
                double v[BPS];
                demap_sym<T, BPS, DM_F32OUT>((T)z.x, (T)z.y, cons, a.c, v);
#pragma unroll
                for (int b = 0; b < BPS; ++b) {
                    const long j = sy * BPS + b;
                    if (j >= j0 && j < j1) L[l * DF_LD + (int)(j - j0)] = (float)v[b];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const long cw = (long)tile * WAVE + lane;
            for (int k = k0; k < k1; ++k) {
                float v[6];
#pragma unroll
                for (int cc = 0; cc < 6; ++cc) {
                    const int j = a.src[(long)(cc < 4 ? cc : cc + 2) * N + k];
                    v[cc] = (j >= 0 && j < a.n_avail && cw < B) ? L[lane * DF_LD + (int)(j - j0)] : 0.0f;
                }
                X[(long)k * WAVE + lane] = make_float4(v[0], v[1], v[2], v[3]);
                Z[(long)k * WAVE + lane] = make_float2(v[4], v[5]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    // the decoder reads the filled planes back through the CU's vector L1, which
    // may hold lines of the buffer's previous tile: publish the stores, invalidate L1
    __device__ __forceinline__ void publish() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
};

template <int ALGO, bool RAG, typename T, int BPS>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(DEC_WPE))) void
k_turbo_decode_syms(DecodeArgs p, const int *__restrict__ perm, const int *__restrict__ inv,
                    const int *__restrict__ used, FusedDemapArgs fa) {
    __shared__ uint32_t epi[WAVES_PER_BLOCK * 2 * WAVE];
    __shared__ T cons[DM_TAB];
    __shared__ float L[WAVES_PER_BLOCK * WAVE * DF_LD];
    load_table<T, BPS>(cons, reinterpret_cast<const T *>(fa.cons_g), fa.c);
    __syncthreads();
    DemapPro<T, BPS> pro{fa, p.B, cons, L + (threadIdx.x >> 6) * WAVE * DF_LD};
    turbo_decode_tiles<ALGO, RAG>(p, perm, inv, used, nullptr, nullptr, epi, pro);
}

// ---- self-tests of the demapper's exact shortcuts (tdec_selftest) -------------------
// which 0: sqrt_1_2 against sqrtf and against the correctly rounded f64 square
// root rounded to f32 (innocuous double rounding for sqrt) for every f32 in
// [1, 2]; which 1 / 2: cabs_fin against npm::cabs_np (f32 / f64) on n
// splitmix64 bit patterns taken as finite (re, im) pairs, every exponent.
// bad[0] counts differing results, bad[1] the items evaluated.
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(BLOCK) void k_selftest(int which, long long n, unsigned long long seed,
                                                    unsigned long long *bad) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    if (which == 0) {
        const float x = __uint_as_float(0x3F800000u + (unsigned)i);
        const unsigned a = __float_as_uint(sqrt_1_2<float>(x));
        ok = a == __float_as_uint(sqrtf(x)) && a == __float_as_uint((float)sqrt((double)x));
    } else if (which == 1) {
        const unsigned long long r = splitmix64(seed + 2 * (unsigned long long)i);
        float re = __uint_as_float((unsigned)r), im = __uint_as_float((unsigned)(r >> 32));
        if (!isfinite(re)) re = 1.5f;
        if (!isfinite(im)) im = -0.75f;
        ok = __float_as_uint(cabs_fin<float>(re, im)) == __float_as_uint(cabs_np<float>(re, im)) &&
             __float_as_uint(cabs_fin<float, true>(re, im)) == __float_as_uint(cabs_np<float>(re, im));
    } else if (which == 3) {
        // log-MAP primitives outside the captured tables: every f32 t >= 48 (bit
        // patterns 0x42400000 .. 0x7F800000 = +inf, n ignored) gives 0 <= 2^-t <= 2^-39
        // (256 * 2^-t is absorbed by any sum >= 1 - 2^-23), with 2^-inf = +0; item 0 also
        // checks NaN -> NaN for both instructions and log2(1) = 0.
        const float t = __uint_as_float(0x42400000u + (unsigned)i);
        const float e = hw_exp2(-t);
        ok = e >= 0.0f && e <= 0x1p-39f && (t != INFINITY || __float_as_uint(e) == 0u);
        if (i == 0) {
            const float qn = __uint_as_float(0x7FC00000u);
            ok = ok && hw_exp2(qn) != hw_exp2(qn) && hw_log2(qn) != hw_log2(qn) && __float_as_uint(hw_log2(1.0f)) == 0u;
        }
    } else if (which == 4) {
        // the unscaled sequences (dm_fast) against the compiler's on the demapper's ranges:
        // |z| of (re, im) with exponents in [-64, 16) (a quarter of the items with
        // |im| within a factor 2 of |re|); a / b with |a| in [2^-900, 2^600), b in
        // [2^-8, 2^100); sqrt on [1, 2)
        const unsigned long long r0 = splitmix64(seed + 4 * (unsigned long long)i), r1 = splitmix64(r0),
                                 r2 = splitmix64(r1), r3 = splitmix64(r2);
        auto mk = [](unsigned long long r, int e) {   // random sign and mantissa, exponent e
            return __longlong_as_double((long long)((r & 0x800FFFFFFFFFFFFFull) | ((unsigned long long)(e + 1023) << 52)));
        };
        const int ea = (int)(r2 % 80) - 64;
        const int eb = (r2 >> 8) & 3 ? (int)((r2 >> 16) % 80) - 64 : ea + (int)((r2 >> 24) & 1);
        const double re = mk(r0, ea), im = mk(r1, eb);
        ok = __double_as_longlong(cabs_fin<double, true>(re, im)) == __double_as_longlong(cabs_np<double>(re, im));
        const double a = mk(r0, (int)(r3 % 1500) - 900), b = fabs(mk(r1, (int)((r3 >> 16) % 108) - 8));
        ok = ok && __double_as_longlong(div_nr64(a, b, rcp_nr64(b))) == __double_as_longlong(a / b);
        const double x = __longlong_as_double((long long)((r2 & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull));
        ok = ok && __double_as_longlong(sqrt_1_2_64(x)) == __double_as_longlong(sqrt(x));
        // f32: |z| with exponents in [-64, 16), a / b with |a| in [2^-90, 2^60), b in [2^-8, 2^16)
        auto mkf = [](unsigned r, int e) { return __uint_as_float((r & 0x807FFFFFu) | ((unsigned)(e + 127) << 23)); };
        const float fre = mkf((unsigned)r0, ea), fim = mkf((unsigned)(r0 >> 32), eb);
        ok = ok && __float_as_uint(cabs_fin<float, true>(fre, fim)) == __float_as_uint(cabs_np<float>(fre, fim));
        const float fa = mkf((unsigned)r1, (int)(r3 % 150) - 90), fb = fabsf(mkf((unsigned)(r1 >> 32), (int)((r3 >> 16) % 24) - 8));
        ok = ok && __float_as_uint(div_nr32(fa, fb, rcp_nr32(fb))) == __float_as_uint(fa / fb);
    } else {
        double re = __longlong_as_double((long long)splitmix64(seed + 2 * (unsigned long long)i));
        double im = __longlong_as_double((long long)splitmix64(seed + 2 * (unsigned long long)i + 1));
        if (!isfinite(re)) re = 1.5;
        if (!isfinite(im)) im = -0.75;
        ok = __double_as_longlong(cabs_fin<double>(re, im)) == __double_as_longlong(cabs_np<double>(re, im)) &&
             __double_as_longlong(cabs_fin<double, true>(re, im)) == __double_as_longlong(cabs_np<double>(re, im));
    }
    if (!ok) atomicAdd(bad, 1ull);
    const unsigned long long act = __ballot(1);   // bad[1]: items evaluated (a launch that did not run fails)
    if ((threadIdx.x & (WAVE - 1)) == (unsigned)__ffsll((long long)act) - 1) atomicAdd(bad + 1, (unsigned long long)__popcll(act));
}

// The log-MAP primitives' exact outputs (test infrastructure: the oracle's
// tables, oracle/tdec_oracle.c orc_set_trans): out[i] = v_exp_f32(-t) (which 0)
// or v_log_f32(w) (which 1) of the f32 whose bit pattern is lo + i.
__global__ __launch_bounds__(BLOCK) void k_trans_table(int which, unsigned lo, long long n, float *out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = __uint_as_float(lo + (unsigned)i);
    out[i] = which == 0 ? hw_exp2(-x) : hw_log2(x);
}

// ---- pilot-aided channel estimation (build-defined) ----------------------
// A framed burst of S data symbols: J = ceil(S / dlen) data segments between J + 1 pilot
// blocks of plen symbols, P0 D0 P1 D1 ... D(J-1) PJ, T = S + (J + 1) plen positions; segment
// j holds data symbols [j dlen, min((j + 1) dlen, S)), L_j of them.  One block per row of
// [B][T] complex64 frames, all arithmetic f64 without contraction, every order fixed:
//   block gain  hp[j] = (nr / e, ni / e) over i = 0 .. plen-1 in turn, sums from 0.0:
//               nr += yr*pr + yi*pi,  ni += yi*pr - yr*pi,  e += pr*pr + pi*pi
//   residual    q_j = sum_i (dr*dr + di*di), d = y_i - (hr*pr - hi*pi, hr*pi + hi*pr)
//   row noise   nv = max_py((q_0 + q_1 + ...) / ((J + 1)(plen - 1)), floor)   (plen >= 2)
//   data u of segment j, a = hp[j], b = hp[j + 1]:
//               w = (double)(2u + plen + 1) / (double)(2 (plen + L_j))   (mean: w = 0.5)
//               h = (float2)(ar + w (br - ar), ai + w (bi - ai)); (0, 0) if a or b is exactly 0
//   EQ:         eq_symbol(y, h, nv_r) -> z, nv_sym;   else y and h are written as they are.
// Thread t forms the gains (and residuals) of pilot blocks t, t + BLOCK, ... into LDS and
// thread 0 adds the residuals in block order, so a row's values depend on neither B nor the
// grid.  The frame is read 8 bytes at a time (T is odd in general: no row alignment to
// speak of); with `vec` (the host checks that every output has the same address modulo 16)
// a thread owns the two symbols of one aligned 16-byte slot of each output row and stores
// them at once, the row's first or last symbol alone where the slot straddles the row's end.
struct CsiArgs {
    const float2 *frames;                      // [B][T]
    const float2 *pilots;                      // [(J + 1) plen]
    int S, plen, dlen, J, T;
    int mean;                                  // 1: w = 0.5
    int estimate;                              // 1: form q_j and the row's nv
    int nv_src;                                // the equaliser's nv_r: 0 nv, 1 nvs[r], 2 the estimate
    int vec, odd0;                             // 16-byte stores; the outputs' base is 8 modulo 16
    double nv, floor_nv;
    const double *nvs;                         // [B]
    float2 *z;                                 // [B][S]: z (EQ) or the stripped y
    double *nv_sym;                            // [B][S] (EQ)
    float2 *h;                                 // [B][S] (nullable with EQ)
    double *nv_out;                            // [B] (nullable)
};

template <bool EQ>
__global__ __launch_bounds__(BLOCK) void k_csi_pilots(CsiArgs a) {
    extern __shared__ __attribute__((aligned(16))) double csi_lds[];
    const int nb = a.J + 1;
    double2 *hp = reinterpret_cast<double2 *>(csi_lds);   // [nb]
    double *q = csi_lds + 2 * nb;                         // [nb], then the row's nv
    const long r = blockIdx.x;
    const float2 *row = a.frames + r * (long)a.T;
    for (int j = threadIdx.x; j < nb; j += BLOCK) {
        // block j starts behind j segments, all full but perhaps the last: at S + J plen for j = J
        const long t0 = j < a.J ? (long)j * (a.plen + a.dlen) : (long)a.S + (long)a.J * a.plen;
        const float2 *y = row + t0, *p = a.pilots + (long)j * a.plen;
        double nr = 0.0, ni = 0.0, e = 0.0;
        for (int i = 0; i < a.plen; ++i) {
            const double yr = (double)y[i].x, yi = (double)y[i].y, pr = (double)p[i].x, pi = (double)p[i].y;
            nr += yr * pr + yi * pi;
            ni += yi * pr - yr * pi;
            e += pr * pr + pi * pi;
        }
        const double hr = nr / e, hi = ni / e;
        hp[j] = make_double2(hr, hi);
        if (a.estimate) {
            double qq = 0.0;
            for (int i = 0; i < a.plen; ++i) {
                const double pr = (double)p[i].x, pi = (double)p[i].y;
                const double dr = (double)y[i].x - (hr * pr - hi * pi), di = (double)y[i].y - (hr * pi + hi * pr);
                qq += dr * dr + di * di;
            }
            q[j] = qq;
        }
    }
    __syncthreads();
    if (a.estimate) {   // uniform
        if (threadIdx.x == 0) {
            double sum = q[0];
            for (int j = 1; j < nb; ++j) sum += q[j];
            const double mean = sum / (double)((long)nb * (a.plen - 1));
            const double v = (a.floor_nv > mean) ? a.floor_nv : mean;
            q[nb] = v;
            if (a.nv_out) a.nv_out[r] = v;
        }
        __syncthreads();
    }
    const double nv_r = a.nv_src == 2 ? q[nb] : (a.nv_src == 1 ? a.nvs[r] : a.nv);
    struct Sym {
        float2 y, h;
    };
    auto at = [&](int s) -> Sym {   // 0 <= s < S
        const int j = s / a.dlen, u = s - j * a.dlen;
        const int L = min(a.dlen, a.S - j * a.dlen);
        const float2 y = row[(long)s + (long)(j + 1) * a.plen];
        const double2 A = hp[j], Bq = hp[j + 1];
        const double w = a.mean ? 0.5 : (double)(2 * u + a.plen + 1) / (double)(2 * (a.plen + L));
        float2 h = make_float2((float)(A.x + w * (Bq.x - A.x)), (float)(A.y + w * (Bq.y - A.y)));
        if ((A.x == 0.0 && A.y == 0.0) || (Bq.x == 0.0 && Bq.y == 0.0)) h = make_float2(0.0f, 0.0f);
        return Sym{y, h};
    };
    const long o = r * (long)a.S;
    if (a.vec) {
        // slot k of the row: symbols 2k - a0 and 2k - a0 + 1, a0 = 1 when the row starts in the
        // upper half of a 16-byte slot
        const int a0 = (int)((o + a.odd0) & 1);
        const int n_slots = (a.S + a0 + 1) / 2;
        for (int k = threadIdx.x; k < n_slots; k += BLOCK) {
            const int s0 = 2 * k - a0;
            if (s0 >= 0 && s0 + 1 < a.S) {
                const Sym u0 = at(s0), u1 = at(s0 + 1);
                if constexpr (EQ) {
                    const EqOut e0 = eq_symbol(u0.y, u0.h, nv_r), e1 = eq_symbol(u1.y, u1.h, nv_r);
                    *reinterpret_cast<float4 *>(a.z + o + s0) = make_float4(e0.zr, e0.zi, e1.zr, e1.zi);
                    *reinterpret_cast<double2 *>(a.nv_sym + o + s0) = make_double2(e0.nv, e1.nv);
                    if (a.h) *reinterpret_cast<float4 *>(a.h + o + s0) = make_float4(u0.h.x, u0.h.y, u1.h.x, u1.h.y);
                } else {
                    *reinterpret_cast<float4 *>(a.z + o + s0) = make_float4(u0.y.x, u0.y.y, u1.y.x, u1.y.y);
                    *reinterpret_cast<float4 *>(a.h + o + s0) = make_float4(u0.h.x, u0.h.y, u1.h.x, u1.h.y);
                }
            } else {
                const int s = s0 >= 0 ? s0 : s0 + 1;   // the row's last symbol, or its first
                const Sym u0 = at(s);
                if constexpr (EQ) {
                    const EqOut e0 = eq_symbol(u0.y, u0.h, nv_r);
                    a.z[o + s] = make_float2(e0.zr, e0.zi);
                    a.nv_sym[o + s] = e0.nv;
                    if (a.h) a.h[o + s] = u0.h;
                } else {
                    a.z[o + s] = u0.y;
                    a.h[o + s] = u0.h;
                }
            }
        }
    } else {
        for (int s = threadIdx.x; s < a.S; s += BLOCK) {
            const Sym u0 = at(s);
            if constexpr (EQ) {
                const EqOut e0 = eq_symbol(u0.y, u0.h, nv_r);
                a.z[o + s] = make_float2(e0.zr, e0.zi);
                a.nv_sym[o + s] = e0.nv;
                if (a.h) a.h[o + s] = u0.h;
            } else {
                a.z[o + s] = u0.y;
                a.h[o + s] = u0.h;
            }
        }
    }
}

}  // namespace tdec
