/*
 * tdec.h -- C ABI of the MI355X (gfx950) DVB-RCS2 duo-binary turbo decoder.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (poriya219/modulations, dvb_rcs2_turbo.py) has no FFI layer: its boundary is
 * the Python API of the module.  Each entry point below states which reference
 * interface it replaces; modulations_amd/dvb_rcs2_turbo.py binds them with
 * ctypes (INTEGRATION.md shows the binding a maintainer would add to the
 * reference module itself).
 *
 * Conventions
 *   - Plain pointers and sizes only.  Row-major, batch-major [B][...].
 *   - Entry points without a _dev suffix take HOST pointers and are
 *     synchronous.  _dev entry points take DEVICE pointers and a hipStream_t
 *     (passed as void*), are stream-ordered, never allocate and never
 *     synchronise once tdec_reserve() has sized the workspace.
 *   - B = 0 (an empty batch) is a no-op that returns 0; the buffers may then be
 *     null.  B < 0 is TDEC_EINVAL.
 *   - Return 0 on success, a negative TDEC_E* code otherwise;
 *     tdec_last_error() (thread-local) says why.  No exception crosses the ABI.
 *   - A handle is bound to one device.  Calls on different handles may run
 *     concurrently from different host threads.
 *   - LLR sign: LLR = log P(0)/P(1) (positive -> bit 0), as the decoder of the
 *     reference (dvb_rcs2_turbo.py:533-535).
 */
#ifndef TDEC_H
#define TDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdec_ctx tdec_t;

enum {
    TDEC_OK = 0,
    TDEC_EINVAL = -1,       /* bad argument (bad N, period, tables, null pointer) -> ValueError */
    TDEC_ESHORT = -2,       /* LLR vector shorter than the de-puncture walk     -> IndexError */
    TDEC_ENOMEM = -3,       /* device allocation failed                          -> MemoryError */
    TDEC_EHIP = -4,         /* HIP runtime error                                 -> RuntimeError */
    TDEC_EUNSUPPORTED = -5, /* trellis tables other than the DVB-RCS2 16-state CRSC */
    TDEC_EITER = -6,        /* iterations < 1 (the reference raises UnboundLocalError) */
    TDEC_ECAPACITY = -7     /* _dev call larger than tdec_reserve()                */
};

enum { TDEC_ALGO_MAXLOG = 0, TDEC_ALGO_LOGMAP = 1 };

/* Codec construction: replaces DVBRCS2_Turbo.__init__ (dvb_rcs2_turbo.py:288-309)
 * for the decode side.  punct = [4][4] uint8 (rows W1, Y1, W2, Y2; columns the
 * pattern phase, PUNCTURE_PATTERNS :21-26), period in 1..4.  perm / inv_perm =
 * int32[n_couples] (the reference's self.perm / self.inv_perm, :311-325).
 * tables = int32[5][16][4]: next_state, out_W, out_Y, prev_state, prev_input
 * (:327-396); anything but the DVB-RCS2 trellis returns TDEC_EUNSUPPORTED. */
int tdec_create(int device, int n_couples, int period, const uint8_t *punct, int iterations, int algo,
                const int32_t *perm, const int32_t *inv_perm, const int32_t *tables, tdec_t **out);
void tdec_destroy(tdec_t *h);
const char *tdec_last_error(void);

/* LLRs one decode reads (the de-puncture walk, :476-487). */
long tdec_llr_len(const tdec_t *h);

/* One SISO pass over B codewords: replaces bcjr_max_log_map
 * (dvb_rcs2_turbo.py:116-281; historic name bcjr_decode_circular).
 * All arrays [B][n_couples], host memory.  Outputs f64 extrinsics. */
int tdec_siso_batch(tdec_t *h, int B, const float *LcA, const float *LcB, const float *LcW, const float *LcY,
                    const double *LaA, const double *LaB, double sf, double *LeA, double *LeB);

/* The same SISO with float64 channel LLRs: bcjr_max_log_map as numba
 * specialises it for float64 Lc arrays (dvb_rcs2_turbo.py:135-160, 267-268:
 * in_A = Lc_A + La_A and the parity terms formed from the unrounded f64
 * values, the extrinsic subtracting the f64 sum).  Float32 inputs widened to
 * f64 give exactly tdec_siso_batch's results. */
int tdec_siso_batch_f64(tdec_t *h, int B, const double *LcA, const double *LcB, const double *LcW,
                        const double *LcY, const double *LaA, const double *LaB, double sf, double *LeA,
                        double *LeB);

/* The per-call form of the same SISO (one bcjr_max_log_map call is one row):
 * tdec_siso_staging returns a page-locked buffer owned by the handle, of 8
 * slots of *slot_bytes each (LcA, LcB, LcW, LcY, LaA, LaB, LeA, LeB: [rows][N]
 * rows of 8-byte elements; float32 channel LLRs fill the first half of their
 * slot).  The caller writes the six inputs there, calls tdec_siso_staged for B
 * <= rows rows and reads LeA / LeB back from the buffer: no argument pointers,
 * no host-side copies in the library.  The buffer stays valid until a later
 * tdec_siso_staging call asks for more rows, or tdec_destroy. */
int tdec_siso_staging(tdec_t *h, int rows, void **buf, size_t *slot_bytes);
int tdec_siso_staged(tdec_t *h, int B, int lc_f64, double sf);
/* Staged calls that waited for their rows' completion flags longer than the
 * library's time limit and ended by a stream synchronisation instead (a
 * diagnostic: the flags live in coherent host memory, so this stays 0). */
int tdec_siso_stats(const tdec_t *h, long *flag_fallbacks);

/* Full turbo decode of B codewords: replaces DVBRCS2_Turbo.decode
 * (dvb_rcs2_turbo.py:464-537; historic name turbo_decode).  llr rows of
 * llr_stride floats (>= tdec_llr_len), bits int32[B][2N] (A, B interleaved as
 * :534-535), lfinal (nullable) f64[B][2N] = Lc + La + Le1 (:529-530). */
int tdec_decode_batch(tdec_t *h, int B, const float *llr, long llr_stride, int32_t *bits, double *lfinal);

/* Pinned (page-locked) host memory for the host-pointer entry points: copies
 * from / to it go straight to the DMA engines, where pageable memory is staged
 * through the runtime's own pinned buffers.  No reference counterpart (numpy
 * buffers are pageable); DVBRCS2_Turbo.host_buffer() wraps it. */
int tdec_host_alloc(size_t bytes, void **out);
void tdec_host_free(void *p);

/* ---- device-pointer, stream-ordered API (what bench.py and multi-GPU use) ---- */

/* Size the workspace for batches of up to max_batch codewords. */
int tdec_reserve(tdec_t *h, int max_batch);
/* Bytes of the de-punctured plane buffer for B codewords.  Layout (opaque to
 * callers): per 64-codeword tile, [N][64] float4 {A, B, W1, Y1} followed by
 * [N][64] float2 {W2, Y2} -- 24 B per trellis step and codeword. */
size_t tdec_planes_bytes(const tdec_t *h, int B);
int tdec_depuncture_dev(tdec_t *h, int B, const float *d_llr, long llr_stride, float *d_planes, void *stream);
int tdec_decode_planes_dev(tdec_t *h, int B, const float *d_planes, int32_t *d_bits, double *d_lfinal,
                           void *stream);
int tdec_decode_batch_dev(tdec_t *h, int B, const float *d_llr, long llr_stride, int32_t *d_bits,
                          double *d_lfinal, void *stream);
/* Pipelining (no reference counterpart): enqueue on `stream` a one-wave kernel
 * that completes once h's most recent throughput decode launch (enqueued before
 * this call, on any stream) has handed out its last tiles, so work queued after
 * it on `stream` -- the next batch's demap -- is dispatched into the slots the
 * decoder's retiring waves free instead of competing with the decoder's grid
 * placement.  No-op before the first such launch; returns after ~2 s at most. */
int tdec_tail_gate(tdec_t *h, void *stream);

/* ---- early termination (no reference counterpart) ----
 * The same decodes with a hard-decision-aided stopping rule per codeword: the
 * iterations at scaling 0.7 run as in the reference; after each of them the
 * decisions ((f64(Lc) + La) + Le1) < 0 of all 2N bits are compared with the
 * previous iteration's (before the first: Lc < 0), and once none changed the
 * next iteration is the final one (scaling 1.0).  n_iter (nullable, int32[B])
 * receives the iterations run, in 2..iterations (1 when iterations = 1).  A
 * row's bits and lfinal are exactly those of the plain entry point on a handle
 * created with iterations = n_iter[row].
 * These calls run on the frame decoder (one codeword per workgroup) for every
 * B, in stream-ordered launches of at most tdec_es_capacity() codewords; they
 * return TDEC_EUNSUPPORTED where it is unavailable (TDEC_FRAME=0 in the
 * environment, or a block whose LDS plan does not fit).  The first call sizes
 * the frame workspace if tdec_reserve has not; later calls never allocate
 * (tdec_decode_batch_es_dev also sizes the handle's plane buffer for one
 * launch on first use). */
int tdec_decode_batch_es(tdec_t *h, int B, const float *llr, long llr_stride, int32_t *bits, double *lfinal,
                         int32_t *n_iter);
int tdec_decode_planes_es_dev(tdec_t *h, int B, const float *d_planes, int32_t *d_bits, double *d_lfinal,
                              int32_t *d_n_iter, void *stream);
int tdec_decode_batch_es_dev(tdec_t *h, int B, const float *d_llr, long llr_stride, int32_t *d_bits,
                             double *d_lfinal, int32_t *d_n_iter, void *stream);
/* Codewords one early-stop launch takes with the handle's current workspace (a
 * multiple of 64; 0 before it is sized), or a negative TDEC_E* code. */
int tdec_es_capacity(tdec_t *h);
/* 1 when the early-stop entry points can serve blocks of n_couples couples in
 * this process (host only: no handle, no device call), else 0. */
int tdec_early_stop_available(int n_couples);

/* The same rule on the throughput tile decoder (64 codewords per wave, one per
 * lane): a lane leaves the iterations on its own, the wave goes
 * on to its next tile once its 64 codewords have ended.  Same outputs, bit for
 * bit, as the calls above (max-log and log-MAP); d_lfinal / d_n_iter nullable.
 * For batches: every block size of the tables (N > 805 included), independent
 * of TDEC_FRAME.  Capacity as tdec_decode_planes_dev / tdec_decode_batch_dev:
 * tdec_reserve(max_batch) first, a larger _dev call is TDEC_ECAPACITY and writes
 * nothing; the host-pointer call reserves and chunks like tdec_decode_batch
 * (TDEC_HOST_CHUNK).  With iterations = 1 this is the plain decode, n_iter = 1.
 * TDEC_ES_TILE_WAVES in the environment (read per call) caps the persistent
 * waves of a launch (diagnostics and tests). */
int tdec_decode_batch_es_tile(tdec_t *h, int B, const float *llr, long llr_stride, int32_t *bits, double *lfinal,
                              int32_t *n_iter);
int tdec_decode_planes_es_tile_dev(tdec_t *h, int B, const float *d_planes, int32_t *d_bits, double *d_lfinal,
                                   int32_t *d_n_iter, void *stream);
int tdec_decode_batch_es_tile_dev(tdec_t *h, int B, const float *d_llr, long llr_stride, int32_t *d_bits,
                                  double *d_lfinal, int32_t *d_n_iter, void *stream);

/* The same rule on the throughput decoder with finished lanes refilled (DESIGN.md
 * §8.3): a lane whose codeword has ended takes the next undecoded codeword of the
 * batch, so a wave's trips (one iteration of its 64 lanes each) follow the sum of
 * the iteration counts, not the per-tile maximum.  Same outputs, bit for bit, as
 * the calls above (max-log and log-MAP); d_lfinal / d_n_iter nullable; every block
 * size of the tables, independent of TDEC_FRAME; B = 0 is a no-op; with
 * iterations = 1 this is the plain decode, n_iter = 1.
 * Each persistent wave decodes from a plane buffer of its own (one 64-codeword
 * tile: tdec_planes_bytes(h, 64) per wave), which only tdec_reserve_es_refill
 * allocates, beside everything tdec_reserve(max_batch) sizes.  The _dev calls never
 * allocate or synchronise: one beyond what tdec_reserve_es_refill covered is
 * TDEC_ECAPACITY and writes nothing.  The host-pointer call reserves for itself
 * and chunks like tdec_decode_batch (TDEC_HOST_CHUNK).  TDEC_ES_TILE_WAVES (read
 * per call) caps the persistent waves of these launches too.
 * Refill order: at the top of every trip the wave claims as many consecutive
 * row indices from the launch's queue as it has free lanes (lanes whose codeword
 * has ended, or that never had one), and the free lanes take them in ascending
 * lane order; indices >= B leave a lane idle for the rest of the launch.  With
 * one wave that order makes `trips` a function of the rows' iteration counts alone.
 * tdec_es_refill_stats (a diagnostic, like tdec_siso_stats) waits for the device
 * and returns, summed over the waves of the handle's most recent refill launch,
 * the trips run and the codewords handed to lanes (= that launch's B); zeros
 * before the first such launch. */
int tdec_reserve_es_refill(tdec_t *h, int max_batch);
int tdec_decode_batch_es_refill(tdec_t *h, int B, const float *llr, long llr_stride, int32_t *bits, double *lfinal,
                                int32_t *n_iter);
int tdec_decode_planes_es_refill_dev(tdec_t *h, int B, const float *d_planes, int32_t *d_bits, double *d_lfinal,
                                     int32_t *d_n_iter, void *stream);
int tdec_decode_batch_es_refill_dev(tdec_t *h, int B, const float *d_llr, long llr_stride, int32_t *d_bits,
                                    double *d_lfinal, int32_t *d_n_iter, void *stream);
int tdec_es_refill_stats(const tdec_t *h, long *trips, long *refills);

/* Soft demapper: compute_llr (test_sdr_with_coding.py:200-225) over any
 * labelled constellation (label i = bits MSB first).  syms: n_sym complex
 * values (f32 pairs, or f64 pairs when sym_f64); cons: M points (host memory,
 * f32 or f64 pairs).  Arithmetic dtype = f64 if either is f64.  div_f32: the
 * (min_d0 - min_d1) / noise_var division stays float32 (numpy >= 2 with a
 * Python-float noise_var).  sign = +1 reference sign (positive -> bit 1),
 * -1 decoder sign.  Output f64[n_sym * bps]. */
int tdec_demap_dev(int device, const void *d_syms, int sym_f64, long n_sym, const void *cons, int cons_f64,
                   int M, int bps, double noise_var, int div_f32, int sign, double *d_llr, void *stream);
int tdec_demap(int device, const void *syms, int sym_f64, long n_sym, const void *cons, int cons_f64, int M,
               int bps, double noise_var, int div_f32, int sign, double *llr);

/* Log-MAP (exact log-sum) soft demapper (build-defined, no reference
 * counterpart): with d_i = |s - c_i|^2 and nv = max(noise_var,
 * 0.005),
 *   llr_b = sign * clip(log sum_{bit_b(i)=1} exp(-d_i/nv) - log sum_{bit_b(i)=0} exp(-d_i/nv), -30, +30)
 * of which the demapper above is the max-log approximation.  Same arguments,
 * dtype rule, sign and output as tdec_demap_dev / tdec_demap, without div_f32
 * (the result is defined by a tolerance, not by numpy's operation order);
 * a NaN or infinite symbol gives NaN for each of its bits. */
int tdec_demap_logmap_dev(int device, const void *d_syms, int sym_f64, long n_sym, const void *cons, int cons_f64,
                          int M, int bps, double noise_var, int sign, double *d_llr, void *stream);
int tdec_demap_logmap(int device, const void *syms, int sym_f64, long n_sym, const void *cons, int cons_f64, int M,
                      int bps, double noise_var, int sign, double *llr);

/* The fixed-signature demapper of SURVEY §8(b) over the reference's built-in
 * Gray constellations (BPSK/QPSK/8PSK/16QAM: test_sdr_with_coding.py:25-100;
 * 64QAM/256QAM: sdr_modem.py:168-207): compute_llr(syms, mod, noise_var)
 * (:200-225) of n_sym complex64 symbols (host f32 pairs) with noise_var given
 * as a Python float would be, then rounded to f32 as decode() rounds its input
 * (dvb_rcs2_turbo.py:466).  sign +1 = reference sign, -1 = decoder sign.
 * llr_out: float[n_sym * bps]. */
enum { TDEC_MOD_BPSK = 0, TDEC_MOD_QPSK = 1, TDEC_MOD_8PSK = 2, TDEC_MOD_16QAM = 3, TDEC_MOD_64QAM = 4,
       TDEC_MOD_256QAM = 5 };
int tdec_demap_batch(int device, int mod, int sign, const float *syms_iq, long n_sym, float noise_var,
                     float *llr_out);
/* The label-ordered table of a built-in constellation (what compute_llr builds,
 * :207-208): M points as (re, im) double pairs in iq[2*M]; *is_f64 = 1 when
 * numpy's table is complex128 (QPSK), else every value is a float32.
 * Returns M, or a negative TDEC_E* code.  Host only (no device call). */
int tdec_constellation(int mod, double *iq, int *is_f64);

/* Fused demap -> de-puncture for the decoder: B codewords of S complex64
 * symbols each ([B][S]); LLR j of a codeword = bit j of its symbol stream
 * (zero-padded / truncated to the decoder's LLR count as
 * test_sdr_with_coding.py:474-478), decoder sign, rounded to f32 as decode()
 * does (:466).  Writes the plane buffer consumed by tdec_decode_planes_dev. */
int tdec_demap_planes_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                          int bps, double noise_var, int div_f32, float *d_planes, void *stream);
/* The same planes from the log-MAP demapper (tdec_demap_logmap_dev with
 * sign = -1, rounded to f32). */
int tdec_demap_planes_logmap_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64,
                                 int M, int bps, double noise_var, float *d_planes, void *stream);

/* Per-row noise variance: a receiver estimates each burst's noise
 * variance from that burst's own symbols (test_sdr_with_coding.py:459-471), so a
 * batch of B bursts has B values.  These calls keep them in device memory, one
 * f64 per row of the [B][S] symbols, so estimate -> demap -> decode is queued on
 * one stream with no host round trip.
 *
 * tdec_noise_var_dev: the decision-directed estimate of :459-467 for each row of
 * complex64 symbols (build-defined: the f64 mean, where numpy's is an f32
 * pairwise mean):
 *   d_nv[r] = max_py(mean_s min_m |s - c_m|^2, floor),  max_py(a, b) = (b > a) ? b : a
 * (Python's max(nv, 0.02): a NaN mean stays NaN; a NaN or infinite symbol makes
 * its row's value NaN).  The minimum is taken over dx*dx + dy*dy of the f64
 * differences; a row's value does not depend on B.
 *
 * tdec_demap_rows_dev / _logmap_dev: tdec_demap_dev / tdec_demap_logmap_dev
 * over B rows of S symbols, row r with noise_var = d_noise_var[r] (floored at
 * 0.005 on the device as the scalar calls floor it on the host); d_llr is
 * f64[B][S * bps].  tdec_demap_planes_nv_dev / _logmap_nv_dev: the same for
 * tdec_demap_planes_dev / tdec_demap_planes_logmap_dev (same ordering on the
 * handle, table upload and decline list; after tdec_reserve they neither
 * allocate nor synchronise).  Row r of each is, bit for bit, row r of the scalar
 * call given noise_var = d_noise_var[r]; a NaN value gives that row NaN LLRs.
 * Conventions as the scalar calls: B = 0 is a no-op, null or negative arguments
 * are TDEC_EINVAL.  The handle-less calls share tdec_demap_dev's table cache.
 * There is no per-row form of the one-launch tdec_demap_decode_dev below: it
 * measured slower than the two launches and is not the default. */
int tdec_noise_var_dev(int device, const float *d_syms, int B, int S, const void *cons, int cons_f64, int M,
                       double floor, double *d_nv, void *stream);
int tdec_demap_rows_dev(int device, const void *d_syms, int sym_f64, int B, int S, const void *cons, int cons_f64,
                        int M, int bps, const double *d_noise_var, int div_f32, int sign, double *d_llr,
                        void *stream);
int tdec_demap_rows_logmap_dev(int device, const void *d_syms, int sym_f64, int B, int S, const void *cons,
                               int cons_f64, int M, int bps, const double *d_noise_var, int sign, double *d_llr,
                               void *stream);
int tdec_demap_planes_nv_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                             int bps, const double *d_noise_var, int div_f32, float *d_planes, void *stream);
int tdec_demap_planes_logmap_nv_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64,
                                    int M, int bps, const double *d_noise_var, float *d_planes, void *stream);

/* Per-symbol noise variance (flat fading with known gains): a
 * received sample y = h x + n equalised to z = y / h has the noise variance
 * nv / |h|^2, so every symbol of a faded burst has its own.  These calls read one
 * f64 per symbol from a device array d_noise_var[B][S], S the launch's symbols per
 * row (tdec_equalize_dev below writes it).
 *
 * tdec_symnv_demap_dev / _logmap_dev: tdec_demap_rows_dev / _logmap_dev with
 * symbol (r, s) demapped at noise_var = d_noise_var[r * S + s] (floored at 0.005
 * on the device); d_llr is f64[B][S * bps].  tdec_symnv_demap_planes_dev /
 * tdec_symnv_demap_planes_logmap_dev: the same for tdec_demap_planes_dev /
 * tdec_demap_planes_logmap_dev (same ordering on the handle, table upload and
 * decline list; after tdec_reserve they neither allocate nor synchronise); the
 * value belongs to the symbol, so the label bits of a couple that come from two
 * symbols each take their own symbol's.  The LLRs of symbol (r, s) are, bit for
 * bit, what the scalar call gives that symbol with noise_var =
 * d_noise_var[r * S + s]: a NaN value gives that symbol NaN LLRs, +inf what the
 * scalar call gives at +inf (zero LLRs for a finite symbol: an erasure).
 * Conventions as the per-row calls: B = 0 is a no-op, null or negative arguments
 * are TDEC_EINVAL. */
int tdec_symnv_demap_dev(int device, const void *d_syms, int sym_f64, int B, int S, const void *cons, int cons_f64,
                        int M, int bps, const double *d_noise_var, int div_f32, int sign, double *d_llr,
                        void *stream);
int tdec_symnv_demap_logmap_dev(int device, const void *d_syms, int sym_f64, int B, int S, const void *cons,
                               int cons_f64, int M, int bps, const double *d_noise_var, int sign, double *d_llr,
                               void *stream);
int tdec_symnv_demap_planes_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                              int bps, const double *d_noise_var, int div_f32, float *d_planes, void *stream);
int tdec_symnv_demap_planes_logmap_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64,
                                     int M, int bps, const double *d_noise_var, float *d_planes, void *stream);

/* The equaliser in front of them (build-defined).  d_y: received
 * symbols, complex64 [B][S]; d_h: channel gains, complex64 [B][ceil(S / coh)],
 * coh >= 1: symbol s of row r uses h[r][s / coh] (coh = 1: per-symbol gains,
 * coh >= S: one gain per burst).  Noise variance of y: d_noise_var[r] (f64 [B] on
 * the device, tdec_noise_var_dev's output or the caller's) when d_noise_var is not
 * null, else the host value noise_var.  Outputs d_z complex64 [B][S] and d_nv_sym
 * f64 [B][S].  All in f64 without contraction:
 *   g = hr*hr + hi*hi,  z = ((float)((yr*hr + yi*hi) / g), (float)((yi*hr - yr*hi) / g)),
 *   nv_sym = nv_r / g   (no floor: the demapper floors)
 * and where g == 0 or g is not finite the symbol is an erasure: z = 0 + 0j,
 * nv_sym = +inf.  B = 0 or S = 0 is a no-op; null pointers, negative sizes and
 * coh < 1 are TDEC_EINVAL. */
int tdec_equalize_dev(int device, const float *d_y, const float *d_h, int B, int S, int coh, double noise_var,
                      const double *d_noise_var, float *d_z, double *d_nv_sym, void *stream);

/* ---- pilot-aided channel estimation (build-defined) ----
 * A framed burst of S data symbols carries J + 1 pilot blocks of plen symbols around
 * J = ceil(S / dlen) data segments, P0 D0 P1 D1 ... D(J-1) PJ, T = S + (J + 1) plen
 * positions; segment j holds data symbols [j dlen, min((j + 1) dlen, S)), L_j of them (only
 * the last may be short).  d_frames: complex64 [B][T]; d_pilots: the known sequence,
 * complex64 [(J + 1) plen] on the device, shared by all rows, every block of non-zero energy
 * (the caller's to check: a zero-energy block gives a non-finite gain, and so erasures).
 * One launch, one block per row, every sum in f64 without contraction in this order:
 *   hp[j] = (nr / e, ni / e),  over i = 0 .. plen-1 in turn from 0.0:
 *           nr += yr*pr + yi*pi,  ni += yi*pr - yr*pi,  e += pr*pr + pi*pi
 *   q_j   = sum_i (dr*dr + di*di),  d = y_i - (hr*pr - hi*pi, hr*pi + hi*pr)
 *   nv[r] = max_py((q_0 + q_1 + ...) / ((J + 1)(plen - 1)), floor)        (plen >= 2 only)
 *   data u of segment j, a = hp[j], b = hp[j + 1]:
 *           w = (double)(2u + plen + 1) / (double)(2 (plen + L_j)),  TDEC_CSI_MEAN: w = 0.5
 *           h = (float)(ar + w (br - ar)), (float)(ai + w (bi - ai));  0 + 0j when a or b is
 *           exactly zero (a block that received nothing vouches for neither neighbour)
 * then z and nv_sym are tdec_equalize_dev's for (y, h, nv_r): complex64 [B][S] and f64
 * [B][S], erasures (z = 0, nv_sym = +inf) where |h|^2 is zero or not finite, so a
 * non-finite pilot erases the segments it borders.  nv_r is d_nv_rows_in[r] (f64 [B]) when
 * that is not null, else noise_var when it is not negative (NaN counts as given), else the
 * estimate nv[r].  d_h (nullable): the interpolated gains, complex64 [B][S]; d_nv_out
 * (nullable, plen >= 2): nv[r], f64 [B], formed whichever source equalises.  A row's
 * values depend on neither B nor the grid.  TDEC_EINVAL: a null required pointer; B, S,
 * plen or dlen < 1; an unknown mode; d_nv_out with plen == 1; no noise source (plen == 1,
 * no d_nv_rows_in, noise_var < 0).  TDEC_EUNSUPPORTED: more than 2048 pilot blocks. */
enum { TDEC_CSI_LINEAR = 0, TDEC_CSI_MEAN = 1 };
int tdec_csi_pilots_dev(int device, const float *d_frames, int B, int S, int plen, int dlen, const float *d_pilots,
                        int mode, double noise_var, const double *d_nv_rows_in, double floor, float *d_z,
                        double *d_nv_sym, float *d_h, double *d_nv_out, void *stream);
/* The unfused form: the stripped data d_y complex64 [B][S] and the gains d_h [B][S] (both
 * required), and nv[r] into d_nv_out when asked; tdec_equalize_dev with coh = 1 behind it
 * writes what the fused call writes, bit for bit. */
int tdec_csi_strip_dev(int device, const float *d_frames, int B, int S, int plen, int dlen, const float *d_pilots,
                       int mode, double floor, float *d_y, float *d_h, double *d_nv_out, void *stream);

/* ---- receive diversity: maximal-ratio combining (build-defined) ----
 * R copies of every burst (antennas, or retransmissions of one burst), each through a gain
 * of its own, combined into what tdec_equalize_dev writes for one, so every demapper and
 * decoder behind it is unchanged.  d_y: complex64 [B][R][S]; d_h: complex64
 * [B][R][ceil(S / coh)], coh >= 1 as for tdec_equalize_dev; 1 <= R <= 8; outputs d_z
 * complex64 [B][S] and d_nv_sym f64 [B][S].  All in f64 without contraction, the branches in
 * the order r = 0 .. R-1.  Per branch
 *   g_r = hr*hr + hi*hi,  a_r = yr*hr + yi*hi,  b_r = yi*hr - yr*hi
 * and a branch whose g_r is zero or not finite is skipped (it vouches for nothing).
 * Common noise (d_nv_branches null): nv_b = d_nv_rows[b] (f64 [B]) when that is not null,
 * else noise_var; G, A, Bm are the sums of g_r, a_r, b_r over the live branches,
 *   z = ((float)(A / G), (float)(Bm / G)),  nv_sym = nv_b / G.
 * Per-branch noise (d_nv_branches, f64 [B][R], each branch's pilot estimate for example):
 * the summed terms are g_r / nv_br, a_r / nv_br, b_r / nv_br,
 *   z = ((float)(A / G), (float)(Bm / G)),  nv_sym = 1.0 / G.
 * Each sum starts from the first live branch's term, not from 0.0 (a -0.0 numerator keeps
 * its sign): R = 1 with common noise is tdec_equalize_dev bit for bit.  No live branch, or
 * a G that came out zero or infinite (an overflow; a zero or infinite nv_br): an erasure,
 * z = 0 + 0j, nv_sym = +inf.  A NaN nv_br is no skip: G is NaN and that row's symbols are
 * NaN (§10's convention); a NaN y stays in its own symbol.  No floor: the demapper floors.
 * B = 0 or S = 0 is a no-op.  TDEC_EINVAL, nothing written: null required pointers, negative
 * sizes, coh < 1, R < 1 or R > 8, both noise arrays given. */
int tdec_combine_dev(int device, const float *d_y, const float *d_h, int B, int R, int S, int coh, double noise_var,
                     const double *d_nv_rows, const double *d_nv_branches, float *d_z, double *d_nv_sym, void *stream);

/* Fused soft demap + turbo decode (one launch): what tdec_demap_planes_dev +
 * tdec_decode_planes_dev compute, bit for bit, with each persistent decoder wave
 * demapping its own next tile into a per-wave plane buffer.  Instantiated for
 * the BASELINE configurations: max-log with complex64 tables of 4 or 8 bits per
 * symbol (16QAM, 256QAM) or complex128 with 2 (QPSK), log-MAP with complex64
 * and 3 (8PSK); tdec_fused_available() says whether a (table dtype, bps) pair
 * has one (TDEC_EUNSUPPORTED otherwise).  tdec_reserve_fused sizes the
 * workspace and the per-wave planes for batches of up to max_batch. */
int tdec_reserve_fused(tdec_t *h, int max_batch);
int tdec_fused_available(const tdec_t *h, int cons_f64, int bps);
int tdec_demap_decode_dev(tdec_t *h, int B, const float *d_syms, int S, const void *cons, int cons_f64, int M,
                          int bps, double noise_var, int div_f32, int32_t *d_bits, double *d_lfinal, void *stream);

/* Batched encoder (workload generation): encode (dvb_rcs2_turbo.py:404-462)
 * with the handle's perm, bits uint8[B][2N] -> coded uint8[B][n_out],
 * n_out = the reference encoder's output length. */
int tdec_encode_dev(tdec_t *h, int B, const uint8_t *d_bits, uint8_t *d_coded, void *stream);
long tdec_encoded_len(const tdec_t *h);
/* The drop-in's DVBRCS2_Turbo.encode (dvb_rcs2_turbo.py:404-462) on the HOST
 * (compiled; needs no handle and no GPU): B rows of int32 info bits [2N]
 * (A, B interleaved; row stride bits_stride) -> int32 coded rows (stride
 * out_stride >= the returned length).  punct: [4][4] pattern rows W1, Y1, W2, Y2
 * as tdec_create; perm: int32[N] (any values in [0, N)).  An input
 * (A << 1) | B outside [-4, 3] is TDEC_ESHORT (numpy's IndexError in the
 * reference's next_state lookup; -4..-1 wrap as numpy's negative indices).
 * Returns the coded length per row (> 0) or a negative error code. */
long tdec_encode_host(int n_couples, int period, const uint8_t *punct, const int32_t *perm, long B,
                      const int32_t *bits, long bits_stride, int32_t *out, long out_stride);

/* ---- counter-based workload generation (not a reference API) ----
 * Codeword c of a batch has the GLOBAL index cw0 + c; its info bits and its
 * channel noise are Philox4x32-10 streams keyed by `seed` and counted by that
 * index, so they do not depend on the batch or the number of ranks a job is
 * sharded over.  Info bit j of codeword g is bit j%32 of word (j%128)/32 of
 * philox4x32_10({g_lo, g_hi, j/128, 0x1AF0}, {seed_lo, seed_hi}).
 * Needs n_couples % 4 == 0 and n_couples <= 1024 (every DVB-RCS2 block size). */

/* info bits -> encode (as tdec_encode_dev) -> label-ordered constellation
 * (cons_iq: M = 2^bps host (re, im) float pairs, label = bps coded bits MSB
 * first, the last symbol zero-padded; any other M is TDEC_EINVAL) -> complex AWGN of std-dev sigma per dimension
 * (Box-Muller on philox4x32_10({g_lo, g_hi, s/2, 0x2B0E}, seed), words x, y for even s and
 * z, w for odd s; each uniform is ((x >> 8) + 0.5) 2^-24 in (0, 1], formed in float32, so the
 * largest draw is exactly 1: radius 0, or angle 2 pi).  d_syms:
 * complex64 [B][ceil(n_out / bps)]; d_info (nullable): uint8 [B][2N]. */
int tdec_workload_dev(tdec_t *h, int B, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                      double sigma, float *d_syms, uint8_t *d_info, void *stream);
/* The same over a flat-fading channel: each symbol is h x + n, with
 * the info bits and the noise tdec_workload_dev draws for the same (seed, cw0 + c, s),
 * and the gains are written to d_h, complex64 [B][ceil(S / coh)], S = ceil(n_out / bps):
 * gain block j of a codeword covers its symbols [j * coh, (j + 1) * coh), coh >= 1.
 *   h = sqrt(K / (K + 1)) + sqrt(1 / (K + 1)) * w,  w ~ CN(0, 1)
 * for the Rician factor K = rician_k >= 0 (0: Rayleigh), w by Box-Muller on
 * philox4x32_10({g_lo, g_hi, j/2, 0x3C5D}, seed) with the noise's uniform mapping,
 * 1/2 variance per dimension.  A codeword's gains depend only on its global index. */
int tdec_workload_fading_dev(tdec_t *h, int B, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                             double sigma, double rician_k, int coh, float *d_syms, float *d_h, uint8_t *d_info,
                             void *stream);
/* Frames of that call's output with pilot blocks (the layout of tdec_csi_pilots_dev, DESIGN.md
 * §13).  d_y complex64 [B][S] and d_gains complex64 [B][ceil(S / coh)] as written by
 * tdec_workload_fading_dev with the same cw0, seed and sigma; d_pilots complex64
 * [(J + 1) plen] on the device; d_frames complex64 [B][T]; d_h_true (nullable) complex64
 * [B][T], the gain each position went through.  Data positions copy their symbol.  Pilot i
 * of block j is h p + n: h the gain of data symbol min(j dlen, S - 1), h p formed in f64
 * and rounded to f32, n Box-Muller noise of sigma per dimension on
 * philox4x32_10({g_lo, g_hi, (j plen + i) / 2, 0x4D6C}, seed), the data noise's mapping.
 * cfo_max > 0: position t of global codeword g is then multiplied by exp(j 2 pi f_g t),
 * f_g = cfo_max (2u - 1) cycles per symbol, u = ((x >> 8) + 0.5) 2^-24 of word x of
 * philox4x32_10({g_lo, g_hi, 0, 0x5E7B}, seed); angle and sincospi in f64, the product
 * rounded to f32; d_h_true carries the rotation.  cfo_max == 0: no multiply. */
int tdec_workload_frame_dev(int device, const float *d_y, const float *d_gains, int B, int S, int coh, int plen,
                            int dlen, const float *d_pilots, double sigma, int64_t cw0, uint64_t seed, double cfo_max,
                            float *d_frames, float *d_h_true, void *stream);
/* R receive branches of every codeword: tdec_workload_fading_dev with d_syms
 * complex64 [B][R][S] and d_h complex64 [B][R][ceil(S / coh)], 1 <= R <= 8.  A codeword's info
 * bits (d_info, uint8 [B][2N]) are shared by its branches; branch b draws its noise and its
 * gains with b in the upper 16 bits of the counter's domain word, 0x2B0E | b << 16 and
 * 0x3C5D | b << 16, so the branches are independent, branch 0 is tdec_workload_fading_dev's
 * output bit for bit, and a codeword still depends only on its global index. */
int tdec_workload_branches_dev(tdec_t *h, int B, int R, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                               double sigma, double rician_k, int coh, float *d_syms, float *d_h, uint8_t *d_info,
                               void *stream);
/* tdec_workload_frame_dev over those branches: d_y [B][R][S] and d_gains [B][R][ceil(S / coh)]
 * framed into d_frames (and d_h_true, nullable) complex64 [B][R][T].  Branch b's pilot noise is
 * drawn with 0x4D6C | b << 16; the rotation f_g belongs to the codeword (one oscillator: the
 * domain word 0x5E7B as it is) and is shared by its branches.  Branch 0 is
 * tdec_workload_frame_dev's output bit for bit. */
int tdec_workload_frame_branches_dev(int device, const float *d_y, const float *d_gains, int B, int R, int S, int coh,
                                     int plen, int dlen, const float *d_pilots, double sigma, int64_t cw0, uint64_t seed,
                                     double cfo_max, float *d_frames, float *d_h_true, void *stream);
/* The info bits alone: uint8 [B][2N] of 0/1. */
int tdec_info_bits_dev(tdec_t *h, int B, int64_t cw0, uint64_t seed, uint8_t *d_info, void *stream);
/* Bit errors per codeword of decoded rows (int32 [B][2N], tdec_decode_*) against
 * those info bits: d_errs int32 [B]. */
int tdec_count_errors_dev(tdec_t *h, int B, int64_t cw0, uint64_t seed, const int32_t *d_bits, int32_t *d_errs,
                          void *stream);

/* ---- self-test of the demapper's exact shortcuts (test infrastructure; no
 * reference counterpart): which 0 compares the kernels' [1, 2] square root with
 * sqrtf and the correctly rounded one for every f32 in [1, 2] (n ignored);
 * which 1 / 2 compare the finite-input |z| with numpy's |z| (npm::cabs_np,
 * f32 / f64) on n pseudo-random finite pairs.  *mismatches = differing results. */
int tdec_selftest(int device, int which, long long n, unsigned long long seed, long long *mismatches);
/* which 3 (same entry point): the log-MAP primitives outside the captured
 * tables -- every f32 t >= 48 gives 0 <= v_exp_f32(-t) <= 2^-39 (+0 at t = inf),
 * NaN -> NaN for v_exp_f32 and v_log_f32, v_log_f32(1) = 0 (n, seed ignored).
 * which 4: the demapper's unscaled f64 division / square root (TDEC_DM_FAST64)
 * against the compiler's sequences on n pseudo-random operands of the ranges
 * the demapper meets (|z|, a / b, sqrt on [1, 2]).
 *
 * The exact outputs of the log-MAP primitives (the oracle's tables,
 * oracle/tdec_oracle.c orc_set_trans): out[i] = v_exp_f32(-t) (which 0) or
 * v_log_f32(w) (which 1) for the f32 whose bit pattern is lo_bits + i, i < n;
 * out is a host buffer of n floats. */
int tdec_selftest_trans(int device, int which, uint32_t lo_bits, long long n, float *out);

#ifdef __cplusplus
}
#endif
#endif /* TDEC_H */
