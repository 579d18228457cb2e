// tdec_demap_api.hip -- the soft demapper's host code, included by
// tdec_api.hip behind the decoder's launch helpers: configuration and argument checks, the
// table caches, the flat and plane launchers with their entries, every exported demap
// call, the noise-variance estimator, the equaliser, the combiner, the fused demap + decode call and the
// built-in constellations.  (ConsCache, the device table itself, is a member of the handle
// and stands with the handle's other buffer types in tdec_api.hip.)

namespace {

// compute_llr's configuration: noise_var floored at 0.005 (:202)
static DemapCfg demap_cfg(int M, int div_f32, int sign, double noise_var, int sep) {
    const double nv = (0.005 > noise_var) ? 0.005 : noise_var;
    return DemapCfg{M, div_f32, sign, nv, sep, dm_nv_fast(nv)};
}

// 1 / (nv ln 2): the log-MAP demapper's exponents in bits, once per launch
static double demap_lm_scale(const DemapCfg &c) { return 1.0 / (c.nv * 0.693147180559945309417); }

int check_demap_args(int M, int bps) {
    if (bps < 1 || bps > 8 || M < 1 || M > (1 << bps) || M > 256) return fail(TDEC_EINVAL, "bad constellation size");
    return 0;
}

// ---- tables, launchers and entries -------------------------------------
// The launchers and entries are templates on ROWNV (0: noise_var per launch; 1:
// noise_var[row], 2: noise_var[row][symbol], read on the device).

// The handle-less calls' device table (the caller holds the device's Guard)
int cached_table(int device, const void *cons, int cons_f64, int M, int bps, bool f64, hipStream_t st,
                 ConsCache **out) {
    // Tables are cached per (thread, device) by content and never overwritten
    // while another stream may still read them: a new table takes a fresh slot;
    // only when all slots are taken is the oldest reused, after a device-wide
    // synchronisation.
    constexpr int SLOTS = 8;
    static thread_local std::vector<ConsCache> tbl[16];
    static thread_local int next_victim[16];
    std::vector<ConsCache> &v = tbl[device & 15];
    if (v.empty()) v.reserve(SLOTS);
    ConsCache *hit = nullptr;
    for (auto &c : v)
        if (c.matches(cons, cons_f64, M, bps, f64)) hit = &c;
    if (!hit) {
        if ((int)v.size() < SLOTS) {
            v.emplace_back();
            hit = &v.back();
        } else {
            HIPCHK(hipDeviceSynchronize());
            hit = &v[next_victim[device & 15]++ % SLOTS];
        }
    }
    *out = hit;
    return hit->upload(cons, cons_f64, M, bps, f64, st);
}

// k_demap / k_demap_lm (lm) over n_sym symbols.  With ROWNV the kernels form each row's
// configuration from rn, and the launch's log-MAP scale is not read: 0.0
template <typename T, typename S, int ROWNV>
int launch_demap(bool lm, int bps, const S *d_syms, long n_sym, const T *d_cons, DemapCfg c, RowNv<ROWNV> rn,
                 double *d_llr, hipStream_t st) {
    const dim3 grid((unsigned)((n_sym + BLOCK - 1) / BLOCK));
    const double scale = ROWNV ? 0.0 : demap_lm_scale(c);
    switch (bps) {
#define CASE(K)                                                                                                      \
    case K:                                                                                                          \
        if (lm) hipLaunchKernelGGL((k_demap_lm<T, S, K, ROWNV>), grid, dim3(BLOCK), 0, st, d_syms, n_sym, d_cons, c, \
                                   scale, d_llr, rn);                                                                \
        else hipLaunchKernelGGL((k_demap<T, S, K, ROWNV>), grid, dim3(BLOCK), 0, st, d_syms, n_sym, d_cons, c,       \
                                d_llr, rn);                                                                          \
        break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: return fail(TDEC_EINVAL, "bps must be 1..8");
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// The flat demappers' entry over [B][S] symbols: B = 1 and noise_var for the scalar calls,
// d_nv[row] or d_nv[row][symbol] with ROWNV (c.nv is then the kernels' to fill).  lm: the log-MAP kernels;
// div_f32 is the max-log path's alone
template <int ROWNV>
int demap_dev(bool lm, int device, const void *d_syms, int sym_f64, long B, long S, const void *cons, int cons_f64,
              int M, int bps, double noise_var, const double *d_nv, int div_f32, int sign, double *d_llr,
              void *stream) {
    if (!d_syms || !cons || !d_llr || (ROWNV && !d_nv) || B < 0 || S < 0)
        return fail(TDEC_EINVAL, "bad demap arguments");
    if (int rc = check_demap_args(M, bps)) return rc;
    if (B == 0 || S == 0) return 0;
    Guard g(device);
    const bool f64 = sym_f64 || cons_f64;
    hipStream_t st = (hipStream_t)stream;
    ConsCache *cc = nullptr;
    if (int rc = cached_table(device, cons, cons_f64, M, bps, f64, st, &cc)) return rc;
    const DemapCfg c = demap_cfg(M, lm ? 0 : div_f32, sign, ROWNV ? 0.0 : noise_var, cc->sep);
    RowNv<ROWNV> rn{};
    if constexpr (ROWNV) rn = {d_nv, S};
    const void *tab = cc->buf.p;
    if (f64 && sym_f64)
        return launch_demap(lm, bps, (const double *)d_syms, B * S, (const double *)tab, c, rn, d_llr, st);
    if (f64) return launch_demap(lm, bps, (const float *)d_syms, B * S, (const double *)tab, c, rn, d_llr, st);
    return launch_demap(lm, bps, (const float *)d_syms, B * S, (const float *)tab, c, rn, d_llr, st);
}

// The host-pointer forms: symbols up, the device entry on a stream of its own, LLRs down
int demap_host(bool lm, int device, const void *syms, int sym_f64, long n_sym, const void *cons, int cons_f64,
               int M, int bps, double noise_var, int div_f32, int sign, double *llr) {
    if (!syms || !cons || !llr || n_sym < 0) return fail(TDEC_EINVAL, "bad demap arguments");
    if (int rc = check_demap_args(M, bps)) return rc;
    if (n_sym == 0) return 0;
    Guard g(device);
    const size_t ns = (size_t)n_sym * 2 * (sym_f64 ? 8 : 4), nl = (size_t)n_sym * bps * sizeof(double);
    void *ds = nullptr, *dl = nullptr;
    HIPCHK(hipMalloc(&ds, ns));
    if (hipMalloc(&dl, nl) != hipSuccess) {
        hipFree(ds);
        return fail(TDEC_ENOMEM, "hipMalloc failed");
    }
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    int rc = 0;
    if (hipMemcpyAsync(ds, syms, ns, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(TDEC_EHIP, "memcpy");
    if (!rc) rc = demap_dev<0>(lm, device, ds, sym_f64, 1, n_sym, cons, cons_f64, M, bps, noise_var, nullptr,
                                   div_f32, sign, (double *)dl, st);
    if (!rc && hipMemcpyAsync(llr, dl, nl, hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(TDEC_EHIP, "memcpy");
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(TDEC_EHIP, "demap failed");
    hipStreamDestroy(st);
    hipFree(ds);
    hipFree(dl);
    return rc;
}

// The handle's table, for a launch on st.  Ordered on the handle first: the table may still
// be read on another stream, and a new one overwrites it
int handle_table(tdec_t *h, const void *cons, int cons_f64, int M, int bps, hipStream_t st) {
    if (int rc = order_on(h, st)) return rc;
    return h->cons.upload(cons, cons_f64, M, bps, cons_f64 != 0, st);
}

// One plane-demapper launch over (64-codeword tile, dm_kc-couple chunk) items, a block each:
// k_demap_planes_lm (lm), k_demap_planes<SPLIT> + k_demap_fix (split tables) or k_demap_planes
template <typename TT, int K, int ROWNV>
void launch_planes(bool lm, bool split, tdec_t *h, int B, int S, const float *d_syms, DemapCfg c, float *P,
                   RowNv<ROWNV> rn, hipStream_t st) {
    const long n_avail = std::min<long>((long)S * K, h->llr_len);   // LLRs the symbols provide
    const long n_tiles = n_tiles_of(B), n_items = n_tiles * ((h->N + dm_kc(K) - 1) / dm_kc(K));
    const dim3 grid((unsigned)n_items), fgrid((unsigned)std::max<long>(1, std::min<long>(n_tiles, 1024)));
    const TT *tab = (const TT *)h->cons.buf.p;
    const int *src = h->d_src, *off = h->d_off, *dst = h->d_dst;
    const DemapDecl dd{h->d_decl, h->d_decl_n, h->d_decl_ovf, DM_DECL_CAP};
    if (lm) {   // the scale per launch; with ROWNV the kernel forms each row's: 0.0
        hipLaunchKernelGGL((k_demap_planes_lm<TT, K, ROWNV>), grid, dim3(BLOCK), 0, st, B, h->N, S, d_syms, tab, c,
                           ROWNV ? 0.0 : demap_lm_scale(c), src, off, n_avail, P, n_items, rn);
        return;
    }
    if constexpr (dm_split(K)) {
        if (split) {
            hipLaunchKernelGGL((k_demap_planes<TT, K, true, ROWNV>), grid, dim3(BLOCK), 0, st, B, h->N, S, d_syms, tab, c,
                               src, off, n_avail, P, n_items, dd, rn);
            hipLaunchKernelGGL((k_demap_fix<TT, K, ROWNV>), fgrid, dim3(BLOCK), 0, st, B, h->N, S, d_syms, tab, c, dst,
                               n_avail, P, dd, n_tiles, rn);
            return;
        }
    }
    hipLaunchKernelGGL((k_demap_planes<TT, K, false, ROWNV>), grid, dim3(BLOCK), 0, st, B, h->N, S, d_syms, tab, c, src,
                       off, n_avail, P, n_items, dd, rn);
}

// The plane demappers' entry: noise_var, or d_nv[row] / d_nv[row][symbol] with ROWNV (c.nv is then the kernels'
// to fill).  lm: the log-MAP kernels, which have no div_f32 and no decline list
template <int ROWNV>
int demap_planes(bool lm, tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M, int bps,
                 double noise_var, const double *d_nv, int div_f32, float *d_planes, void *stream) {
    if (!h || B < 0 || !cons) return fail(TDEC_EINVAL, "bad demap arguments");
    if (int rc = check_demap_args(M, bps)) return rc;
    if (B == 0) return 0;
    if (!d_syms || !d_planes || (ROWNV && !d_nv) || S <= 0) return fail(TDEC_EINVAL, "bad demap arguments");
    Guard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = handle_table(h, cons, cons_f64, M, bps, st)) return rc;
    const DemapCfg c = demap_cfg(M, lm ? 0 : div_f32, -1, ROWNV ? 0.0 : noise_var, h->cons.sep);
    RowNv<ROWNV> rn{};
    if constexpr (ROWNV) rn = {d_nv, S};
    const bool split = !lm && dm_split_table(bps, h->cons.sep);
    if (split) {   // the decline list: sized by tdec_reserve / tdec_reserve_fused
        const long n_tiles = n_tiles_of(B);
        if (h->decl_tiles < n_tiles) {
            // an unreserved batch: allocate here, outside any stream capture (hipFree
            // synchronises the device, and a captured graph must not hold a buffer
            // freed by a later regrowth)
            if (capturing(st)) return fail(TDEC_ECAPACITY, "demap batch larger than tdec_reserve() (stream capture)");
            quiesce(h);
            if (int rc = ensure_decl(h, n_tiles)) return rc;
        }
        HIPCHK(hipMemsetAsync(h->d_decl_n, 0, sizeof(unsigned), st));
        HIPCHK(hipMemsetAsync(h->d_decl_ovf, 0, (size_t)n_tiles, st));
    }
    switch (bps) {
#define CASE(K)                                                                                       \
    case K:                                                                                           \
        if (cons_f64) launch_planes<double, K>(lm, split, h, B, S, d_syms, c, d_planes, rn, st);      \
        else launch_planes<float, K>(lm, split, h, B, S, d_syms, c, d_planes, rn, st);                \
        break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: return fail(TDEC_EINVAL, "bps must be 1..8");
    }
    HIPCHK(hipGetLastError());
    return mark_used(h, st);
}

// k_equalize over n_sym symbols; vec: two symbols per thread, 16-byte accesses
template <bool NVROWS>
void launch_equalize(bool vec, const float2 *y, const float2 *hh, long n_sym, int S, int coh, int nh, double nv,
                     const double *nvs, float2 *z, double *nv_sym, hipStream_t st) {
    if (vec) {
        const long n_thr = (n_sym + 1) / 2;
        hipLaunchKernelGGL((k_equalize<NVROWS, true>), dim3((unsigned)((n_thr + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, y,
                           hh, n_sym, S, coh, nh, nv, nvs, z, nv_sym);
    } else {
        hipLaunchKernelGGL((k_equalize<NVROWS, false>), dim3((unsigned)((n_sym + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st,
                           y, hh, n_sym, S, coh, nh, nv, nvs, z, nv_sym);
    }
}

// k_combine over n_sym = B * S combined symbols; NV: the noise source (0 nv,
// 1 nvs[row], 2 nvs[row][branch]); vec: two symbols per thread, 16-byte accesses
template <int NV>
void launch_combine(bool vec, const float2 *y, const float2 *hh, long n_sym, int R, int S, int coh, int nh, double nv,
                    const double *nvs, float2 *z, double *nv_sym, hipStream_t st) {
    if (vec) {
        const long n_thr = n_sym / 2;
        hipLaunchKernelGGL((k_combine<NV, true>), dim3((unsigned)((n_thr + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, y, hh,
                           n_sym, R, S, coh, nh, nv, nvs, z, nv_sym);
    } else {
        hipLaunchKernelGGL((k_combine<NV, false>), dim3((unsigned)((n_sym + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, y, hh,
                           n_sym, R, S, coh, nh, nv, nvs, z, nv_sym);
    }
}

// k_csi_pilots, one block per framed row.  EQ: estimate + equalise into z and
// nv_sym with the row's noise variance from d_nv_rows (when not null), else noise_var (when not
// negative), else the pilots' own estimate; !EQ: the stripped data and the interpolated gains.
// The residual estimate is formed when it is the noise source or d_nv_out asks for it.
constexpr int CSI_MAX_BLOCKS = 2048;   // pilot blocks per row whose gains and residuals LDS holds (48 KiB)
template <bool EQ>
int csi_pilots(int device, const float *d_frames, int B, int S, int plen, int dlen, const float *d_pilots, int mode,
               double noise_var, const double *d_nv_rows, double floor, float *d_z, double *d_nv_sym, float *d_h,
               double *d_nv_out, void *stream) {
    if (B < 1 || S < 1 || plen < 1 || dlen < 1) return fail(TDEC_EINVAL, "csi_pilots: B, S, plen and dlen must be >= 1");
    if (mode != TDEC_CSI_LINEAR && mode != TDEC_CSI_MEAN) return fail(TDEC_EINVAL, "csi_pilots: unknown interpolation mode");
    if (d_nv_out && plen < 2) return fail(TDEC_EINVAL, "csi_pilots: a noise estimate needs plen >= 2");
    const int nv_src = !EQ ? 0 : (d_nv_rows ? 1 : (!(noise_var < 0.0) ? 0 : 2));
    if (nv_src == 2 && plen < 2) return fail(TDEC_EINVAL, "csi_pilots: no noise source (plen == 1 and no noise_var)");
    const int J = (S + dlen - 1) / dlen;
    if (J + 1 > CSI_MAX_BLOCKS) return fail(TDEC_EUNSUPPORTED, "csi_pilots: more than 2048 pilot blocks per burst");
    const long T = (long)S + (long)(J + 1) * plen;
    if (T > INT32_MAX) return fail(TDEC_EINVAL, "csi_pilots: frame too long");
    Guard g(device);
    CsiArgs a{};
    a.frames = reinterpret_cast<const float2 *>(d_frames);
    a.pilots = reinterpret_cast<const float2 *>(d_pilots);
    a.S = S, a.plen = plen, a.dlen = dlen, a.J = J, a.T = (int)T;
    a.mean = mode == TDEC_CSI_MEAN;
    a.estimate = nv_src == 2 || d_nv_out != nullptr;
    a.nv_src = nv_src;
    a.nv = noise_var, a.floor_nv = floor, a.nvs = d_nv_rows;
    a.z = reinterpret_cast<float2 *>(d_z), a.nv_sym = d_nv_sym, a.h = reinterpret_cast<float2 *>(d_h), a.nv_out = d_nv_out;
    // 16-byte stores where every output has the same address modulo 16 (their elements are 8 bytes)
    const uintptr_t z0 = (uintptr_t)d_z & 15;
    a.vec = (z0 & 7) == 0 && (!d_nv_sym || ((uintptr_t)d_nv_sym & 15) == z0) && (!d_h || ((uintptr_t)d_h & 15) == z0);
    a.odd0 = z0 == 8;
    const size_t lds = (3 * (size_t)(J + 1) + 1) * sizeof(double);
    hipLaunchKernelGGL((k_csi_pilots<EQ>), dim3((unsigned)B), dim3(BLOCK), lds, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace

// ---- exported calls ---------------------------------------------------------------------
extern "C" {

int tdec_demap_dev(int device, const void *d_syms, int sym_f64, long n_sym, const void *cons, int cons_f64, int M,
                   int bps, double noise_var, int div_f32, int sign, double *d_llr, void *stream) {
    return demap_dev<0>(false, device, d_syms, sym_f64, 1, n_sym, cons, cons_f64, M, bps, noise_var, nullptr,
                            div_f32, sign, d_llr, stream);
}

int tdec_demap_logmap_dev(int device, const void *d_syms, int sym_f64, long n_sym, const void *cons, int cons_f64,
                          int M, int bps, double noise_var, int sign, double *d_llr, void *stream) {
    return demap_dev<0>(true, device, d_syms, sym_f64, 1, n_sym, cons, cons_f64, M, bps, noise_var, nullptr, 0,
                            sign, d_llr, stream);
}

int tdec_demap(int device, const void *syms, int sym_f64, long n_sym, const void *cons, int cons_f64, int M, int bps,
               double noise_var, int div_f32, int sign, double *llr) {
    return demap_host(false, device, syms, sym_f64, n_sym, cons, cons_f64, M, bps, noise_var, div_f32, sign, llr);
}

int tdec_demap_logmap(int device, const void *syms, int sym_f64, long n_sym, const void *cons, int cons_f64, int M,
                      int bps, double noise_var, int sign, double *llr) {
    return demap_host(true, device, syms, sym_f64, n_sym, cons, cons_f64, M, bps, noise_var, 0, sign, llr);
}

int tdec_demap_planes_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                          int bps, double noise_var, int div_f32, float *d_planes, void *stream) {
    return demap_planes<0>(false, h, B, d_syms, S, cons, cons_f64, M, bps, noise_var, nullptr, div_f32, d_planes,
                               stream);
}

int tdec_demap_planes_logmap_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                                 int bps, double noise_var, float *d_planes, void *stream) {
    return demap_planes<0>(true, h, B, d_syms, S, cons, cons_f64, M, bps, noise_var, nullptr, 0, d_planes, stream);
}

// per-row noise variance
int tdec_demap_rows_dev(int device, const void *d_syms, int sym_f64, int B, int S, const void *cons, int cons_f64,
                        int M, int bps, const double *d_noise_var, int div_f32, int sign, double *d_llr,
                        void *stream) {
    return demap_dev<1>(false, device, d_syms, sym_f64, B, S, cons, cons_f64, M, bps, 0.0, d_noise_var, div_f32, sign,
                           d_llr, stream);
}

int tdec_demap_rows_logmap_dev(int device, const void *d_syms, int sym_f64, int B, int S, const void *cons,
                               int cons_f64, int M, int bps, const double *d_noise_var, int sign, double *d_llr,
                               void *stream) {
    return demap_dev<1>(true, device, d_syms, sym_f64, B, S, cons, cons_f64, M, bps, 0.0, d_noise_var, 0, sign, d_llr,
                           stream);
}

int tdec_demap_planes_nv_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                             int bps, const double *d_noise_var, int div_f32, float *d_planes, void *stream) {
    return demap_planes<1>(false, h, B, d_syms, S, cons, cons_f64, M, bps, 0.0, d_noise_var, div_f32, d_planes,
                              stream);
}

int tdec_demap_planes_logmap_nv_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64,
                                    int M, int bps, const double *d_noise_var, float *d_planes, void *stream) {
    return demap_planes<1>(true, h, B, d_syms, S, cons, cons_f64, M, bps, 0.0, d_noise_var, 0, d_planes, stream);
}

// per-symbol noise variance (flat fading)
int tdec_symnv_demap_dev(int device, const void *d_syms, int sym_f64, int B, int S, const void *cons, int cons_f64,
                        int M, int bps, const double *d_noise_var, int div_f32, int sign, double *d_llr,
                        void *stream) {
    return demap_dev<2>(false, device, d_syms, sym_f64, B, S, cons, cons_f64, M, bps, 0.0, d_noise_var, div_f32, sign,
                        d_llr, stream);
}

int tdec_symnv_demap_logmap_dev(int device, const void *d_syms, int sym_f64, int B, int S, const void *cons,
                               int cons_f64, int M, int bps, const double *d_noise_var, int sign, double *d_llr,
                               void *stream) {
    return demap_dev<2>(true, device, d_syms, sym_f64, B, S, cons, cons_f64, M, bps, 0.0, d_noise_var, 0, sign, d_llr,
                        stream);
}

int tdec_symnv_demap_planes_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                              int bps, const double *d_noise_var, int div_f32, float *d_planes, void *stream) {
    return demap_planes<2>(false, h, B, d_syms, S, cons, cons_f64, M, bps, 0.0, d_noise_var, div_f32, d_planes, stream);
}

int tdec_symnv_demap_planes_logmap_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64,
                                     int M, int bps, const double *d_noise_var, float *d_planes, void *stream) {
    return demap_planes<2>(true, h, B, d_syms, S, cons, cons_f64, M, bps, 0.0, d_noise_var, 0, d_planes, stream);
}

int tdec_noise_var_dev(int device, const float *d_syms, int B, int S, const void *cons, int cons_f64, int M,
                       double floor, double *d_nv, void *stream) {
    if (B < 0 || !cons) return fail(TDEC_EINVAL, "bad noise_var arguments");
    int bps = 1;
    while (bps < 8 && (1 << bps) < M) ++bps;
    if (int rc = check_demap_args(M, bps)) return rc;
    if (B == 0) return 0;
    if (!d_syms || !d_nv || S <= 0) return fail(TDEC_EINVAL, "bad noise_var arguments");
    Guard g(device);
    hipStream_t st = (hipStream_t)stream;
    ConsCache *cc = nullptr;
    if (int rc = cached_table(device, cons, cons_f64, M, bps, cons_f64 != 0, st, &cc)) return rc;
    if (cons_f64)
        hipLaunchKernelGGL(k_noise_var<double>, dim3((unsigned)B), dim3(BLOCK), 0, st, d_syms, S,
                           (const double *)cc->buf.p, M, floor, d_nv);
    else
        hipLaunchKernelGGL(k_noise_var<float>, dim3((unsigned)B), dim3(BLOCK), 0, st, d_syms, S,
                           (const float *)cc->buf.p, M, floor, d_nv);
    HIPCHK(hipGetLastError());
    return 0;
}

int tdec_equalize_dev(int device, const float *d_y, const float *d_h, int B, int S, int coh, double noise_var,
                      const double *d_noise_var, float *d_z, double *d_nv_sym, void *stream) {
    if (B < 0 || S < 0 || coh < 1) return fail(TDEC_EINVAL, "bad equalize arguments");
    if (B == 0 || S == 0) return 0;
    if (!d_y || !d_h || !d_z || !d_nv_sym) return fail(TDEC_EINVAL, "bad equalize arguments");
    Guard g(device);
    const long n_sym = (long)B * S;
    const int nh = (S + coh - 1) / coh;
    // 16-byte accesses where y, z and nv_sym all allow them
    const bool vec = (((uintptr_t)d_y | (uintptr_t)d_z | (uintptr_t)d_nv_sym) & 15) == 0;
    const float2 *y = reinterpret_cast<const float2 *>(d_y), *hh = reinterpret_cast<const float2 *>(d_h);
    float2 *z = reinterpret_cast<float2 *>(d_z);
    if (d_noise_var) launch_equalize<true>(vec, y, hh, n_sym, S, coh, nh, 0.0, d_noise_var, z, d_nv_sym, (hipStream_t)stream);
    else launch_equalize<false>(vec, y, hh, n_sym, S, coh, nh, noise_var, nullptr, z, d_nv_sym, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// pilot-aided channel estimation
int tdec_csi_pilots_dev(int device, const float *d_frames, int B, int S, int plen, int dlen, const float *d_pilots,
                        int mode, double noise_var, const double *d_nv_rows_in, double floor, float *d_z,
                        double *d_nv_sym, float *d_h, double *d_nv_out, void *stream) {
    if (!d_frames || !d_pilots || !d_z || !d_nv_sym) return fail(TDEC_EINVAL, "csi_pilots: null pointer");
    return csi_pilots<true>(device, d_frames, B, S, plen, dlen, d_pilots, mode, noise_var, d_nv_rows_in, floor, d_z,
                            d_nv_sym, d_h, d_nv_out, stream);
}

int tdec_csi_strip_dev(int device, const float *d_frames, int B, int S, int plen, int dlen, const float *d_pilots,
                       int mode, double floor, float *d_y, float *d_h, double *d_nv_out, void *stream) {
    if (!d_frames || !d_pilots || !d_y || !d_h) return fail(TDEC_EINVAL, "csi_strip: null pointer");
    return csi_pilots<false>(device, d_frames, B, S, plen, dlen, d_pilots, mode, -1.0, nullptr, floor, d_y, nullptr,
                             d_h, d_nv_out, stream);
}

// receive diversity
int tdec_combine_dev(int device, const float *d_y, const float *d_h, int B, int R, int S, int coh, double noise_var,
                     const double *d_nv_rows, const double *d_nv_branches, float *d_z, double *d_nv_sym, void *stream) {
    if (B < 0 || S < 0 || coh < 1 || R < 1 || R > 8) return fail(TDEC_EINVAL, "bad combine arguments (1 <= R <= 8, coh >= 1)");
    if (d_nv_rows && d_nv_branches) return fail(TDEC_EINVAL, "combine: one noise array at most");
    if (B == 0 || S == 0) return 0;
    if (!d_y || !d_h || !d_z || !d_nv_sym) return fail(TDEC_EINVAL, "bad combine arguments");
    Guard g(device);
    const long n_sym = (long)B * S;
    const int nh = (S + coh - 1) / coh;
    // 16-byte accesses where a pair of symbols stays in its row and y, z and nv_sym all allow them
    const bool vec = S % 2 == 0 && (((uintptr_t)d_y | (uintptr_t)d_z | (uintptr_t)d_nv_sym) & 15) == 0;
    const float2 *y = reinterpret_cast<const float2 *>(d_y), *hh = reinterpret_cast<const float2 *>(d_h);
    float2 *z = reinterpret_cast<float2 *>(d_z);
    hipStream_t st = (hipStream_t)stream;
    if (d_nv_branches) launch_combine<2>(vec, y, hh, n_sym, R, S, coh, nh, 0.0, d_nv_branches, z, d_nv_sym, st);
    else if (d_nv_rows) launch_combine<1>(vec, y, hh, n_sym, R, S, coh, nh, 0.0, d_nv_rows, z, d_nv_sym, st);
    else launch_combine<0>(vec, y, hh, n_sym, R, S, coh, nh, noise_var, nullptr, z, d_nv_sym, st);
    HIPCHK(hipGetLastError());
    return 0;
}

#if TDEC_DM_STATS
// measurement build only: symbols per demap path since the last call (see dm_count)
int tdec_demap_stats(unsigned long long *out) {
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dm_stats), 8 * sizeof(unsigned long long)) != hipSuccess)
        return fail(TDEC_EHIP, "g_dm_stats");
    const unsigned long long z[8] = {};
    hipMemcpyToSymbol(HIP_SYMBOL(g_dm_stats), z, sizeof(z));
    return 0;
}
#endif

// ---- fused demap + decode (k_turbo_decode_syms) ---------------------------------------

// The instantiated (algorithm, symbol dtype, bits per symbol) combinations: the
// BASELINE configurations (QPSK / 16QAM / 256QAM max-log, 8PSK log-MAP); anything
// else runs k_demap_planes + k_turbo_decode.
static const void *fused_kernel(int algo, bool ragged, bool f64, int bps) {
    if (ragged) return nullptr;
    if (algo == 0 && !f64 && bps == 4) return (const void *)k_turbo_decode_syms<0, false, float, 4>;
    if (algo == 0 && !f64 && bps == 8) return (const void *)k_turbo_decode_syms<0, false, float, 8>;
    if (algo == 0 && f64 && bps == 2) return (const void *)k_turbo_decode_syms<0, false, double, 2>;
    if (algo == 1 && !f64 && bps == 3) return (const void *)k_turbo_decode_syms<1, false, float, 3>;
    return nullptr;
}

static int waves_for(const tdec_t *h, int B) { return std::min(n_tiles_of(B), h->max_waves); }

int tdec_reserve_fused(tdec_t *h, int max_batch) {
    if (!h || max_batch < 0) return fail(TDEC_EINVAL, "bad reserve");
    if (max_batch == 0) return 0;
    Guard g(h->device);
    const int w = waves_for(h, max_batch);
    const size_t pw = 2 * (size_t)w * tile_floats(h->N) * sizeof(float);
    if (w > h->ws_waves || pw > h->planes_w.cap) quiesce(h);
    int rc = ensure_ws(h, w);
    if (!rc) rc = h->planes_w.ensure(pw);
    return rc;
}

int tdec_fused_available(const tdec_t *h, int cons_f64, int bps) {
    return h && fused_kernel(h->algo, h->N % win_unstaged(h->algo) != 0, cons_f64 != 0, bps) != nullptr;
}

int tdec_demap_decode_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                          int bps, double noise_var, int div_f32, int32_t *d_bits, double *d_lfinal, void *stream) {
    if (!h || B < 0 || !cons) return fail(TDEC_EINVAL, "bad demap-decode arguments");
    if (int rc = check_demap_args(M, bps)) return rc;
    if (B == 0) return 0;
    if (!d_syms || !d_bits || S <= 0) return fail(TDEC_EINVAL, "bad demap-decode arguments");
    const void *k = fused_kernel(h->algo, h->N % win_unstaged(h->algo) != 0, cons_f64 != 0, bps);
    if (!k) return fail(TDEC_EUNSUPPORTED, "no fused demap-decode kernel for this modulation / algorithm");
    Guard g(h->device);
    const int tiles = n_tiles_of(B);
    int waves = waves_for(h, B);
    if (waves > h->ws_waves || 2 * (size_t)waves * tile_floats(h->N) * sizeof(float) > h->planes_w.cap)
        return fail(TDEC_ECAPACITY, "workspace too small: call tdec_reserve_fused first");
    if (const char *pc = getenv("TDEC_TILE_WAVES")) waves = std::max(1, std::min(waves, atoi(pc)));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = handle_table(h, cons, cons_f64, M, bps, st)) return rc;
    const FusedDemapArgs fa{d_syms, S, std::min<long>((long)S * bps, h->llr_len), (const int *)h->d_src,
                            (const int *)h->d_off, (float *)h->planes_w.p,
                            demap_cfg(M, div_f32, -1, noise_var, h->cons.sep), h->cons.buf.p};
    // no caller's planes (each wave demaps into its own), workgroups of WAVES_PER_BLOCK waves;
    // this launch neither arms the issue-priority slots nor raises the tail flag
    return launch_tiles(h, k, WAVES_PER_BLOCK, B, waves, nullptr, d_bits, d_lfinal, tile_queue(h, tiles, waves, st), 0, st,
                        fa);
}

}  // extern "C"

// ---- built-in Gray constellations and the fixed-signature demapper --------------------
// The label-ordered tables compute_llr builds (test_sdr_with_coding.py:207-208)
// from the reference mappers, with numpy's arithmetic and result dtype:
//   BPSK   2.0 * complex64(b) - 1.0                       (:25-26)          complex64
//   QPSK   complex64(1-2b0 + j(1-2b1)) / np.sqrt(2)        (:31-37)          complex128
//          (numpy divides by the complex128 scalar sqrt(2)+0j with Smith's
//          method: re * (1 / sqrt(2)))
//   8PSK   exp(j * GRAY3[label] * pi / 4) -> complex64    (:45-57)
//   QAM    (2*gray[i] - (L-1)) / sqrt(scale) per axis     (:72-86, sdr_modem.py:142-207) complex64
static int builtin_constellation(int mod, double *iq, int *is_f64) {
    static const int g2[4] = {0, 1, 3, 2}, g3[8] = {0, 1, 3, 2, 6, 7, 5, 4},
                     g4[16] = {0, 1, 3, 2, 6, 7, 5, 4, 12, 13, 15, 14, 10, 11, 9, 8};
    *is_f64 = 0;
    switch (mod) {
    case TDEC_MOD_BPSK:
        for (int i = 0; i < 2; ++i) {
            iq[2 * i] = (double)(2.0f * (float)i - 1.0f);
            iq[2 * i + 1] = 0.0;
        }
        return 2;
    case TDEC_MOD_QPSK: {
        *is_f64 = 1;
        const double scl = 1.0 / (std::sqrt(2.0) + 0.0 * 0.0);
        for (int i = 0; i < 4; ++i) {
            const double re = 1 - 2 * (i >> 1), im = 1 - 2 * (i & 1);
            iq[2 * i] = (re + im * 0.0) * scl;
            iq[2 * i + 1] = (im - re * 0.0) * scl;
        }
        return 4;
    }
    case TDEC_MOD_8PSK:
        for (int i = 0; i < 8; ++i) {
            const double p = g3[i] * M_PI / 4;
            iq[2 * i] = (double)(float)std::cos(p);
            iq[2 * i + 1] = (double)(float)std::sin(p);
        }
        return 8;
    case TDEC_MOD_16QAM:
    case TDEC_MOD_64QAM:
    case TDEC_MOD_256QAM: {
        const int k = mod == TDEC_MOD_16QAM ? 2 : (mod == TDEC_MOD_64QAM ? 3 : 4);
        const int L = 1 << k, scale = k == 2 ? 10 : (k == 3 ? 42 : 170);
        const int *g = k == 2 ? g2 : (k == 3 ? g3 : g4);
        const double sq = std::sqrt((double)scale);
        for (int i = 0; i < L * L; ++i) {
            iq[2 * i] = (double)(float)((double)(2 * g[i >> k] - (L - 1)) / sq);
            iq[2 * i + 1] = (double)(float)((double)(2 * g[i & (L - 1)] - (L - 1)) / sq);
        }
        return L * L;
    }
    default: return fail(TDEC_EINVAL, "unknown modulation id");
    }
}

int tdec_constellation(int mod, double *iq, int *is_f64) {
    if (!iq || !is_f64) return fail(TDEC_EINVAL, "null argument");
    return builtin_constellation(mod, iq, is_f64);
}

int tdec_demap_batch(int device, int mod, int sign, const float *syms_iq, long n_sym, float noise_var,
                     float *llr_out) {
    double tab[512];
    int f64 = 0;
    const int M = builtin_constellation(mod, tab, &f64);
    if (M < 0) return M;
    if (n_sym < 0 || (sign != 1 && sign != -1)) return fail(TDEC_EINVAL, "bad demap arguments");
    int bps = 0;
    while ((1 << bps) < M) ++bps;
    if (n_sym == 0) return 0;
    if (!syms_iq || !llr_out) return fail(TDEC_EINVAL, "bad demap arguments");
    std::vector<float> t32;
    const void *cons = tab;
    if (!f64) {   // complex64 table
        t32.assign(tab, tab + 2 * M);
        cons = t32.data();
    }
    // compute_llr with a Python-float noise_var: the final division stays
    // float32 unless the arithmetic is complex128 (QPSK)
    const double nv = (double)noise_var;
    std::vector<double> l64((size_t)n_sym * bps);
    const int rc = tdec_demap(device, syms_iq, 0, n_sym, cons, f64, M, bps, nv, !f64, sign, l64.data());
    if (rc) return rc;
    for (size_t i = 0; i < l64.size(); ++i) llr_out[i] = (float)l64[i];   // decode()'s f32 cast (:466)
    return 0;
}
