// tdec_workload.hip -- device-side workload generation for the turbo decoder
// (SURVEY §8(d), §8(f) row 1): counter-based info bits, the batched encoder
// (encode, dvb_rcs2_turbo.py:404-462), Gray mapping and complex AWGN, and the
// error counters of a BER point.
//
// Counter-based: every random number is Philox4x32-10 (Random123) of a counter
// that names the codeword by its GLOBAL index, so a codeword's info bits and
// noise do not depend on the batch it was generated in, nor on the number of
// ranks a job is sharded over:
//   info bits   ctr = {cw_lo, cw_hi, 128-bit block, 0x1AF0}, key = seed
//   noise       ctr = {cw_lo, cw_hi, symbol pair,    0x2B0E}, key = seed
//   gains       ctr = {cw_lo, cw_hi, gain-block pair, 0x3C5D}, key = seed   (k_workload_fading)
//   pilot noise ctr = {cw_lo, cw_hi, pilot pair,      0x4D6C}, key = seed   (k_workload_frame)
//   rotation    ctr = {cw_lo, cw_hi, 0,               0x5E7B}, key = seed   (k_workload_frame)
//   gains, 2nd  ctr = {cw_lo, cw_hi, gain-block pair, 0x6F8A}, key = seed   (transmit antenna 1)
// Receive branch b of a codeword draws its noise, gains and pilot noise with
// b in the upper 16 bits of the domain word (0x2B0E | b << 16, ...): branch 0 is the
// streams above; the info bits and the rotation are the codeword's, shared by its branches.
// Retransmission tx of a codeword takes the same tag, tx << 16 (tx <= 65535).
// Info bit j of a codeword is bit j % 32 of word (j % 128) / 32 of block j / 128.
// Noise: Box-Muller, u = (x >> 8 + 0.5) * 2^-24 in (0, 1], formed in float32
// (x >> 8 = 2^24 - 1 rounds to u = 1: radius 0, or angle 2 pi): one complex sample
// per symbol from two words, r = sigma * sqrt(-2 ln u1), theta = 2 pi u2.
//
// Layout (MI355X-first): one wave owns a tile of 64 codewords.  The tile's info
// couples are packed 16 per 32-bit word into LDS, [word][lane] (the encoder
// recursion is serial per codeword, one codeword per lane, and the
// interleaver read inp[perm[i]] is the same word for every lane: conflict
// free).  Everything that touches HBM is done cooperatively by the wave in
// row order -- consecutive lanes write consecutive bytes of one codeword row
// -- through small LDS chunks, so every global access is coalesced:
//   bits in    32 B per (codeword, 16 couples) item, 4 x 8-B loads
//   coded out  4-B stores (byte stores when a row is not a multiple of 4)
//   symbols    8-B complex64 stores, noise generated in the coalesced phase
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace tdec {

struct Philox4 {
    uint32_t x, y, z, w;
};

// Philox4x32-10 (Salmon et al., SC'11; Random123's philox4x32_R(10, ...)).
__host__ __device__ __forceinline__ Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = Philox4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
    }
    return c;
}

constexpr uint32_t INFO_DOMAIN = 0x1AF0u, NOISE_DOMAIN = 0x2B0Eu, FADE_DOMAIN = 0x3C5Du;

__device__ __forceinline__ Philox4 info_block(uint64_t cw, uint32_t blk, uint64_t seed) {
    return philox4x32_10(Philox4{(uint32_t)cw, (uint32_t)(cw >> 32), blk, INFO_DOMAIN}, (uint32_t)seed,
                         (uint32_t)(seed >> 32));
}
__device__ __forceinline__ uint32_t pick(const Philox4 &r, int q) {
    return q == 0 ? r.x : (q == 1 ? r.y : (q == 2 ? r.z : r.w));
}
// info bits (bit 2i = A_i, bit 2i+1 = B_i) -> couple word (inp_i = A<<1 | B at bits 2i+1..2i)
__device__ __forceinline__ uint32_t swap_pairs(uint32_t x) { return ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u); }

constexpr int ENC_MAX_N = 1024;                 // couples the LDS-staged encoder holds (else the row kernel)
constexpr int ENC_NW = ENC_MAX_N / 16;          // couple words per codeword
constexpr int SYM_CHUNK = 64;                   // symbols per lane staged before a coalesced flush
constexpr int OUT_CHUNK = 8;                    // coded words (32 bits) per lane staged before a flush

struct WorkloadArgs {
    int B, N, period, bps, M;
    long n_out;                                 // coded bits per codeword
    int S;                                      // symbols per codeword = ceil(n_out / bps)
    uint64_t cw0, seed;                         // global index of codeword 0 of this batch; generator key
    float sigma;                                // noise std-dev per dimension
    unsigned char punct[16];
    int circ[16];
    const int *perm;
    const uint8_t *bits_in;                     // [B][2N] 0/1 bytes, or null: Philox info bits
    uint8_t *info_out;                          // [B][2N] 0/1 bytes (nullable)
    uint8_t *coded_out;                         // [B][n_out] (nullable)
    float2 *syms;                               // [B][S] complex64 (nullable)
    float2 cons[256];                           // label-ordered constellation (by value: no upload)
};

// Fill the wave's couple words inpw[w][lane] for codewords base .. base+63.
__device__ __forceinline__ void load_couples(const WorkloadArgs &p, long base, uint32_t (*inpw)[64], int lane) {
    const int NW = (p.N + 15) / 16;
    const long row = 2L * p.N;
    if (p.bits_in) {
        for (int t = lane; t < 64 * NW; t += 64) {
            const int l = t / NW, w = t - l * NW;
            uint32_t word = 0;
            if (base + l < p.B) {
                const uint8_t *src = p.bits_in + (base + l) * row + 32L * w;
                const int nb = (int)min(32L, row - 32L * w);   // a multiple of 8: 2N is (N % 4 == 0 or the row kernel)
                for (int c = 0; c < nb; c += 8) {
                    const uint2 v = *reinterpret_cast<const uint2 *>(src + c);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        word |= ((v.x >> (8 * k)) & 1u) << ((c + k) ^ 1);
                        word |= ((v.y >> (8 * k)) & 1u) << ((c + 4 + k) ^ 1);
                    }
                }
            }
            inpw[w][l] = word;
        }
    } else {
        const int NB = (2 * p.N + 127) / 128;    // 128-bit Philox blocks per codeword
        for (int t = lane; t < 64 * NB; t += 64) {
            const int l = t / NB, b = t - l * NB;
            const Philox4 r = info_block(p.cw0 + (uint64_t)(base + l), (uint32_t)b, p.seed);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (4 * b + q < NW) inpw[4 * b + q][l] = swap_pairs(pick(r, q));
        }
    }
    __syncthreads();
    if (p.info_out) {   // 0/1 bytes, 4 per store, row order
        for (int t = lane; t < 64 * NW * 8; t += 64) {
            const int l = t / (NW * 8), r = t - l * (NW * 8), w = r >> 3, q = r & 7;
            const long j = 32L * w + 4 * q;      // first info bit of this store
            if (base + l < p.B && j < row) {
                const uint32_t x = inpw[w][l] >> (4 * q);
                const uint32_t bytes = ((x >> 1) & 1u) | ((x & 1u) << 8) | (((x >> 3) & 1u) << 16) | (((x >> 2) & 1u) << 24);
                *reinterpret_cast<uint32_t *>(p.info_out + (base + l) * row + j) = bytes;
            }
        }
    }
}

__device__ __forceinline__ int inp_at(uint32_t (*inpw)[64], int i, int lane) { return (inpw[i >> 4][lane] >> (2 * (i & 15))) & 3; }

__device__ __forceinline__ int enc_next(int s, int inp) {   // next_state (:357-366)
    const int dk = ((inp >> 1) & 1) ^ (inp & 1) ^ ((s >> 2) & 1) ^ ((s >> 3) & 1);
    return (((s >> 2) & 1) << 3) | (((s >> 1) & 1) << 2) | ((s & 1) << 1) | dk;
}

// Row-order flush of a chunk of coded words outw[w][lane] (w < nw) covering coded
// bits [b0, b0 + 32 nw) of every codeword: one byte per bit.
__device__ __forceinline__ void flush_coded(const WorkloadArgs &p, long base, uint32_t (*outw)[64], int nw, long b0,
                                            int lane) {
    __syncthreads();
    if ((p.n_out & 3) == 0) {
        const int per = nw * 8;                  // 4-byte stores per codeword
        for (int t = lane; t < 64 * per; t += 64) {
            const int l = t / per, r = t - l * per;
            const long j = b0 + 4L * r;
            if (base + l < p.B && j < p.n_out) {
                const uint32_t x = outw[r >> 3][l] >> (4 * (r & 7));
                const uint32_t v = (x & 1u) | (((x >> 1) & 1u) << 8) | (((x >> 2) & 1u) << 16) | (((x >> 3) & 1u) << 24);
                *reinterpret_cast<uint32_t *>(p.coded_out + (base + l) * p.n_out + j) = v;
            }
        }
    } else {
        const int per = nw * 32;
        for (int t = lane; t < 64 * per; t += 64) {
            const int l = t / per, r = t - l * per;
            const long j = b0 + r;
            if (base + l < p.B && j < p.n_out) p.coded_out[(base + l) * p.n_out + j] = (outw[r >> 5][l] >> (r & 31)) & 1u;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ float2 awgn(uint64_t cw, long s, const WorkloadArgs &p, uint32_t domain = NOISE_DOMAIN) {
    const Philox4 r = philox4x32_10(Philox4{(uint32_t)cw, (uint32_t)(cw >> 32), (uint32_t)(s >> 1), domain},
                                    (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const uint32_t a = (s & 1) ? r.z : r.x, b = (s & 1) ? r.w : r.y;
    const float u1 = ((float)(a >> 8) + 0.5f) * 0x1p-24f, u2 = ((float)(b >> 8) + 0.5f) * 0x1p-24f;
    const float rad = p.sigma * sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    return make_float2(rad * cs, rad * sn);
}

// Flat fading (k_workload_fading): gain block j of a codeword covers its
// symbols [j * coh, (j + 1) * coh).  h = los + scat * w, w ~ CN(0, 1) by awgn()'s uniform
// mapping and sincospif form on the gain stream (unit total variance: 1/2 per dimension);
// los = sqrt(K / (K + 1)), scat = sqrt(1 / (K + 1)) for the Rician factor K (0: Rayleigh).
struct FadeArgs {
    float2 *h;                                  // [B][nh] complex64
    int coh, nh;                                // symbols per gain block; nh = ceil(S / coh)
    float los, scat;
};
// BranchArgs: R branches of every codeword, rows [B][R] of syms and h
struct BranchArgs : FadeArgs {
    int R;
};
// TxArgs: transmission tx of every codeword, its noise and gains tagged as
// branch tx's; fade = 0: no gains, x + n
struct TxArgs : FadeArgs {
    int tx, fade;
};
// StbcArgs (include/stbc.h): the Alamouti 2 x R link.  syms rows [B][R] of S2 = S + (S & 1)
// slots, h rows [B][R][2] of nh = ceil(S2 / coh) gains, coh even
struct StbcArgs : FadeArgs {
    int R, S2;
};
// SmArgs (include/sm.h): the multiplexed 2 x R link.  syms rows [B][R] of T = ceil(S / 2)
// slots, h rows [B][R][2] of nh = ceil(T / coh) gains, coh >= 1 in slots
struct SmArgs : FadeArgs {
    int R, T;
};
constexpr uint32_t FADE1_DOMAIN = 0x6F8Au;      // antenna 1's gains (antenna 0's: FADE_DOMAIN, the branch generator's)
__device__ __forceinline__ float2 fade_gain(uint64_t cw, long j, uint64_t seed, const FadeArgs &f,
                                            uint32_t domain = FADE_DOMAIN) {
    const Philox4 r = philox4x32_10(Philox4{(uint32_t)cw, (uint32_t)(cw >> 32), (uint32_t)(j >> 1), domain},
                                    (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t a = (j & 1) ? r.z : r.x, b = (j & 1) ? r.w : r.y;
    const float u1 = ((float)(a >> 8) + 0.5f) * 0x1p-24f, u2 = ((float)(b >> 8) + 0.5f) * 0x1p-24f;
    const float rad = 0.70710678118654752f * sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    return make_float2(f.los + f.scat * (rad * cs), f.scat * (rad * sn));
}

// Copy b of symbol s of codeword cw at row `row` of syms and h: table point x through gain
// block s / coh of the streams tagged b (b << 16 in the domain word) plus that stream's noise
// (n: the untagged sample, which is stream 0's).  A receive branch (BranchArgs) or a
// retransmission (TxArgs): the same tag, hence the same samples.
__device__ __forceinline__ void branch_symbol(const WorkloadArgs &p, const FadeArgs &f, uint64_t cw, long s, float2 x,
                                              float2 n, int b, long row) {
    const long j = s / f.coh;
    const uint32_t tag = (uint32_t)b << 16;
    const float2 g = fade_gain(cw, j, p.seed, f, FADE_DOMAIN | tag);
    const float2 nb = b ? awgn(cw, s, p, NOISE_DOMAIN | tag) : n;
    if (s == j * f.coh) f.h[row * f.nh + j] = g;
    p.syms[row * p.S + s] = make_float2((g.x * x.x - g.y * x.y) + nb.x, (g.x * x.y + g.y * x.x) + nb.y);
}

// The Alamouti link's flush (StbcArgs): the chunk's pairs (x[2m], x[2m+1]), one per item, consecutive
// lanes on consecutive pairs of one codeword.  s0 is even (SYM_CHUNK is), and only a codeword's last
// chunk can have an odd ns: its last pair takes the pad point x[S] = 0.  Per branch b: the two paths'
// effective gains (the raw draws times sqrt(1/2) per component), written by the first pair of their
// block (coh is even: a block starts on an even slot), and the two slots
//   2m:    antenna 0 sends  x[2m],          antenna 1  x[2m+1]
//   2m+1:  antenna 0 sends -conj(x[2m+1]),  antenna 1  conj(x[2m])
// each h0 s0 + h1 s1 in the order include/stbc.h states, plus branch b's noise sample of that slot.
__device__ __forceinline__ float2 stbc_slot(float2 h0, float2 s0, float2 h1, float2 s1, float2 n) {
    return make_float2(((h0.x * s0.x - h0.y * s0.y) + (h1.x * s1.x - h1.y * s1.y)) + n.x,
                       ((h0.x * s0.y + h0.y * s0.x) + (h1.x * s1.y + h1.y * s1.x)) + n.y);
}
__device__ __forceinline__ void flush_stbc(const WorkloadArgs &p, const StbcArgs &f, long base, uint8_t (*lab)[64],
                                           const float2 *cons, int ns, long s0, int lane) {
    const int np = (ns + 1) >> 1;
    for (int t = lane; t < 64 * np; t += 64) {
        const int l = t / np, k = 2 * (t - l * np);
        if (base + l >= p.B) continue;
        const uint64_t cw = p.cw0 + (uint64_t)(base + l);
        const float2 x0 = cons[lab[k][l]], x1 = k + 1 < ns ? cons[lab[k + 1][l]] : make_float2(0.0f, 0.0f);
        const float2 c0 = make_float2(-x1.x, x1.y), c1 = make_float2(x0.x, -x0.y);   // -conj(x1), conj(x0)
        const long s = s0 + k, j = s / f.coh;
        for (int b = 0; b < f.R; ++b) {
            const uint32_t tag = (uint32_t)b << 16;
            const long row = (base + l) * f.R + b;
            float2 g0 = fade_gain(cw, j, p.seed, f, FADE_DOMAIN | tag), g1 = fade_gain(cw, j, p.seed, f, FADE1_DOMAIN | tag);
            g0 = make_float2(g0.x * 0.70710678118654752f, g0.y * 0.70710678118654752f);
            g1 = make_float2(g1.x * 0.70710678118654752f, g1.y * 0.70710678118654752f);
            if (s == j * f.coh) {
                f.h[(row * 2 + 0) * f.nh + j] = g0;
                f.h[(row * 2 + 1) * f.nh + j] = g1;
            }
            float2 *out = p.syms + row * f.S2 + s;   // s + 1 < S2: S2 is even
            out[0] = stbc_slot(g0, x0, g1, x1, awgn(cw, s, p, NOISE_DOMAIN | tag));
            out[1] = stbc_slot(g0, c0, g1, c1, awgn(cw, s + 1, p, NOISE_DOMAIN | tag));
        }
    }
}

// The multiplexed link's flush (SmArgs): the chunk's pairs (x[2m], x[2m+1]), one slot per item, consecutive
// lanes on consecutive slots of one codeword (s0 is even, as above; the last pair of an odd S sends 0 from
// antenna 1).  Per branch b: the Alamouti link's effective gains of block m / coh, written by the block's
// first slot, and slot m = h0 x[2m] + h1 x[2m+1] in stbc_slot's order plus branch b's noise sample at
// symbol index m.
__device__ __forceinline__ void flush_sm(const WorkloadArgs &p, const SmArgs &f, long base, uint8_t (*lab)[64],
                                         const float2 *cons, int ns, long s0, int lane) {
    const int np = (ns + 1) >> 1;
    for (int t = lane; t < 64 * np; t += 64) {
        const int l = t / np, k = 2 * (t - l * np);
        if (base + l >= p.B) continue;
        const uint64_t cw = p.cw0 + (uint64_t)(base + l);
        const float2 x0 = cons[lab[k][l]], x1 = k + 1 < ns ? cons[lab[k + 1][l]] : make_float2(0.0f, 0.0f);
        const long m = (s0 + k) >> 1, j = m / f.coh;
        for (int b = 0; b < f.R; ++b) {
            const uint32_t tag = (uint32_t)b << 16;
            const long row = (base + l) * f.R + b;
            float2 g0 = fade_gain(cw, j, p.seed, f, FADE_DOMAIN | tag), g1 = fade_gain(cw, j, p.seed, f, FADE1_DOMAIN | tag);
            g0 = make_float2(g0.x * 0.70710678118654752f, g0.y * 0.70710678118654752f);
            g1 = make_float2(g1.x * 0.70710678118654752f, g1.y * 0.70710678118654752f);
            if (m == j * f.coh) {
                f.h[(row * 2 + 0) * f.nh + j] = g0;
                f.h[(row * 2 + 1) * f.nh + j] = g1;
            }
            p.syms[row * f.T + m] = stbc_slot(g0, x0, g1, x1, awgn(cw, m, p, NOISE_DOMAIN | tag));
        }
    }
}

// Row-order flush of a chunk of symbol labels lab[k][lane] (k < ns): symbols
// [s0, s0 + ns) of every codeword, table point + AWGN, complex64.  FADE: h x + AWGN, and
// the first symbol of each gain block writes its gain.  F = BranchArgs: f.R independently faded
// and independently noisy copies of each symbol, branch b at row (codeword) * R + b.
template <bool FADE, typename F>
__device__ __forceinline__ void flush_syms(const WorkloadArgs &p, const F &f, long base, uint8_t (*lab)[64],
                                           const float2 *cons, int ns, long s0, int lane) {
    __syncthreads();
    if constexpr (std::is_same<F, StbcArgs>::value) {
        flush_stbc(p, f, base, lab, cons, ns, s0, lane);
        __syncthreads();
        return;
    }
    if constexpr (std::is_same<F, SmArgs>::value) {
        flush_sm(p, f, base, lab, cons, ns, s0, lane);
        __syncthreads();
        return;
    }
    for (int t = lane; t < 64 * ns; t += 64) {
        const int l = t / ns, k = t - l * ns;
        if (base + l < p.B) {
            const uint64_t cw = p.cw0 + (uint64_t)(base + l);
            const float2 x = cons[lab[k][l]], n = awgn(cw, s0 + k, p);
            if constexpr (std::is_same<F, BranchArgs>::value) {
                for (int b = 0; b < f.R; ++b) branch_symbol(p, f, cw, s0 + k, x, n, b, (base + l) * f.R + b);
            } else if constexpr (std::is_same<F, TxArgs>::value) {
                if (f.fade) branch_symbol(p, f, cw, s0 + k, x, n, f.tx, base + l);
                else {
                    const float2 nt = f.tx ? awgn(cw, s0 + k, p, NOISE_DOMAIN | (uint32_t)f.tx << 16) : n;
                    p.syms[(base + l) * (long)p.S + s0 + k] = make_float2(x.x + nt.x, x.y + nt.y);
                }
            } else if constexpr (FADE) {
                const long s = s0 + k, j = s / f.coh;
                const float2 g = fade_gain(cw, j, p.seed, f);
                if (s == j * f.coh) f.h[(base + l) * (long)f.nh + j] = g;
                p.syms[(base + l) * (long)p.S + s] =
                    make_float2((g.x * x.x - g.y * x.y) + n.x, (g.x * x.y + g.y * x.x) + n.y);
            } else {
                p.syms[(base + l) * (long)p.S + s0 + k] = make_float2(x.x + n.x, x.y + n.y);
            }
        }
    }
    __syncthreads();
}

// One wave per 64-codeword tile (block = 1 wave: no cross-wave barriers).
template <bool FADE, typename F = FadeArgs>
__device__ __forceinline__ void workload_tile(const WorkloadArgs &p, const F &f) {
    __shared__ uint32_t inpw[ENC_NW][64];
    __shared__ uint32_t outw[OUT_CHUNK][64];
    __shared__ uint8_t lab[SYM_CHUNK][64];
    __shared__ float2 cons[256];
    const int lane = threadIdx.x;
    const long base = (long)blockIdx.x * 64;
    for (int m = lane; m < p.M; m += 64) cons[m] = p.cons[m];
    load_couples(p, base, inpw, lane);
    if (!p.coded_out && !p.syms) return;
    // pass 1: final states from 0 (:433-437 of _encode_component); circular start (:438)
    int s1 = 0, s2 = 0;
    for (int i = 0; i < p.N; ++i) {
        s1 = enc_next(s1, inp_at(inpw, i, lane));
        s2 = enc_next(s2, inp_at(inpw, p.perm[i], lane));
    }
    s1 = p.circ[s1];
    s2 = p.circ[s2];
    // pass 2: the coded stream in output order (:449-460), one bit at a time
    uint32_t acc = 0;
    int nacc = 0, nw = 0;           // coded-word accumulator; words staged in outw
    long b0 = 0;                    // first coded bit of the staged chunk
    int lbl = 0, nl = 0, ns = 0;    // symbol label accumulator (MSB first); labels staged in lab
    long s0 = 0;
    auto emit = [&](int bit) {
        if (p.coded_out) {
            acc |= (uint32_t)bit << nacc;
            if (++nacc == 32) {
                outw[nw][lane] = acc;
                acc = 0;
                nacc = 0;
                if (++nw == OUT_CHUNK) {
                    flush_coded(p, base, outw, nw, b0, lane);
                    b0 += 32L * nw;
                    nw = 0;
                }
            }
        }
        if (p.syms) {
            lbl = (lbl << 1) | bit;
            if (++nl == p.bps) {
                lab[ns][lane] = (uint8_t)lbl;
                lbl = 0;
                nl = 0;
                if (++ns == SYM_CHUNK) {
                    flush_syms<FADE, F>(p, f, base, lab, cons, ns, s0, lane);
                    s0 += ns;
                    ns = 0;
                }
            }
        }
    };
    for (int i = 0; i < p.N; ++i) {
        const int ph = i % p.period;
        const int i1 = inp_at(inpw, i, lane), i2 = inp_at(inpw, p.perm[i], lane);
        const int dk1 = ((i1 >> 1) & 1) ^ (i1 & 1) ^ ((s1 >> 2) & 1) ^ ((s1 >> 3) & 1);
        const int dk2 = ((i2 >> 1) & 1) ^ (i2 & 1) ^ ((s2 >> 2) & 1) ^ ((s2 >> 3) & 1);
        emit((i1 >> 1) & 1);
        emit(i1 & 1);
        if (p.punct[0 * 4 + ph]) emit(dk1 ^ (s1 & 1) ^ ((s1 >> 1) & 1) ^ ((s1 >> 3) & 1));
        if (p.punct[1 * 4 + ph]) emit(dk1 ^ ((s1 >> 1) & 1) ^ ((s1 >> 2) & 1) ^ ((s1 >> 3) & 1));
        if (p.punct[2 * 4 + ph]) emit(dk2 ^ (s2 & 1) ^ ((s2 >> 1) & 1) ^ ((s2 >> 3) & 1));
        if (p.punct[3 * 4 + ph]) emit(dk2 ^ ((s2 >> 1) & 1) ^ ((s2 >> 2) & 1) ^ ((s2 >> 3) & 1));
        s1 = enc_next(s1, i1);
        s2 = enc_next(s2, i2);
    }
    if (p.coded_out) {
        if (nacc) outw[nw++][lane] = acc;
        if (nw) flush_coded(p, base, outw, nw, b0, lane);
    }
    if (p.syms) {
        if (nl) lab[ns++][lane] = (uint8_t)(lbl << (p.bps - nl));   // zero pad of the last symbol
        if (ns) flush_syms<FADE, F>(p, f, base, lab, cons, ns, s0, lane);
    }
}

// ---- row encoder (encode, :404-462): one codeword per thread, for the N the staged encoder does not hold ----
struct EncodeArgs {
    int B, N, period;
    long n_out;
    unsigned char punct[16];
    int circ[16];
    const int *perm;
    const uint8_t *bits;
    uint8_t *coded;
};

__device__ __forceinline__ int next_rt(int s, int inp) {
    const int dk = ((inp >> 1) & 1) ^ (inp & 1) ^ ((s >> 2) & 1) ^ ((s >> 3) & 1);
    return (((s >> 2) & 1) << 3) | (((s >> 1) & 1) << 2) | ((s & 1) << 1) | dk;
}

__global__ __launch_bounds__(BLOCK) void k_encode(EncodeArgs p) {
    const long cw = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (cw >= p.B) return;
    const uint8_t *u = p.bits + cw * 2 * p.N;
    uint8_t *o = p.coded + cw * p.n_out;
    int s1 = 0, s2 = 0;
    for (int i = 0; i < p.N; ++i) {
        const int j = p.perm[i];
        s1 = next_rt(s1, (u[2 * i] << 1) | u[2 * i + 1]);
        s2 = next_rt(s2, (u[2 * j] << 1) | u[2 * j + 1]);
    }
    s1 = p.circ[s1];
    s2 = p.circ[s2];
    long q = 0;
    for (int i = 0; i < p.N; ++i) {
        const int j = p.perm[i], ph = i % p.period;
        const int i1 = (u[2 * i] << 1) | u[2 * i + 1], i2 = (u[2 * j] << 1) | u[2 * j + 1];
        const int dk1 = ((i1 >> 1) & 1) ^ (i1 & 1) ^ ((s1 >> 2) & 1) ^ ((s1 >> 3) & 1);
        const int dk2 = ((i2 >> 1) & 1) ^ (i2 & 1) ^ ((s2 >> 2) & 1) ^ ((s2 >> 3) & 1);
        o[q++] = u[2 * i];
        o[q++] = u[2 * i + 1];
        if (p.punct[0 * 4 + ph]) o[q++] = dk1 ^ (s1 & 1) ^ ((s1 >> 1) & 1) ^ ((s1 >> 3) & 1);
        if (p.punct[1 * 4 + ph]) o[q++] = dk1 ^ ((s1 >> 1) & 1) ^ ((s1 >> 2) & 1) ^ ((s1 >> 3) & 1);
        if (p.punct[2 * 4 + ph]) o[q++] = dk2 ^ (s2 & 1) ^ ((s2 >> 1) & 1) ^ ((s2 >> 3) & 1);
        if (p.punct[3 * 4 + ph]) o[q++] = dk2 ^ ((s2 >> 1) & 1) ^ ((s2 >> 2) & 1) ^ ((s2 >> 3) & 1);
        s1 = next_rt(s1, i1);
        s2 = next_rt(s2, i2);
    }
}

__global__ __launch_bounds__(64) void k_workload(WorkloadArgs p) { workload_tile<false>(p, FadeArgs{}); }

// Bit errors of decoded rows against the counter-based info bits: one wave per
// codeword, each lane 4 consecutive bits (one 16-B load) per sweep.
__global__ __launch_bounds__(64) void k_count_errors(int B, int N, uint64_t cw0, uint64_t seed, const int32_t *bits,
                                                     int32_t *errs) {
    const int lane = threadIdx.x;
    const long cw = blockIdx.x;
    if (cw >= B) return;
    const int row = 2 * N;
    const int4 *r4 = reinterpret_cast<const int4 *>(bits + cw * (long)row);
    int e = 0;
    for (int j = 4 * lane; j < row; j += 256) {
        const Philox4 r = info_block(cw0 + (uint64_t)cw, (uint32_t)(j >> 7), seed);
        const uint32_t w = pick(r, (j >> 5) & 3) >> (j & 31);
        int4 v;
        if (j + 4 <= row && (row & 3) == 0) v = r4[j >> 2];
        else {
            const int32_t *q = bits + cw * (long)row + j;
            v = make_int4(q[0], j + 1 < row ? q[1] : 0, j + 2 < row ? q[2] : 0, j + 3 < row ? q[3] : 0);
        }
        e += (v.x != (int)(w & 1u)) + (j + 1 < row && v.y != (int)((w >> 1) & 1u)) +
             (j + 2 < row && v.z != (int)((w >> 2) & 1u)) + (j + 3 < row && v.w != (int)((w >> 3) & 1u));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    if (lane == 0) errs[cw] = e;
}


// k_workload with flat fading: the same bits and the same noise, each symbol h x + n, and
// the gains written to f.h.
__global__ __launch_bounds__(64) void k_workload_fading(WorkloadArgs p, FadeArgs f) { workload_tile<true>(p, f); }

// k_workload_fading over R receive branches (f: BranchArgs).  A template, so
// that the kernel-order manifest places it: a plain kernel would stand among the
// non-template ones and move those behind it.
template <typename F> __global__ __launch_bounds__(64) void k_workload_faded(WorkloadArgs p, F f) {
    workload_tile<true, F>(p, f);
}

// ---- framing with pilot blocks (k_workload_frame) --------------------------
// k_workload_fading's symbols y [B][S] and gains [B][nh] framed as P0 D0 P1 D1 ... D(J-1) PJ
// (k_csi_pilots' layout), one thread per frame position.  Data positions copy their symbol.
// Pilot i of block j is h p + n: h the gain of data symbol min(j dlen, S - 1), p =
// pilots[j plen + i], h p formed in f64 and rounded to f32 once per component, n Box-Muller
// noise of sigma per dimension in awgn()'s form on a stream of its own,
//   pilot noise ctr = {cw_lo, cw_hi, (j plen + i) / 2, 0x4D6C}, key = seed
// CFO: position t is then multiplied by exp(j 2 pi f t), f = cfo_max (2u - 1) cycles per
// symbol with u = (x >> 8 + 0.5) 2^-24 of
//   rotation    ctr = {cw_lo, cw_hi, 0, 0x5E7B}, key = seed
// the angle 2 (f t) and sincospi in f64, each product component rounded to f32 once.
// h_true (nullable) is the gain each position went through, the rotation included.
constexpr uint32_t PILOT_DOMAIN = 0x4D6Cu, CFO_DOMAIN = 0x5E7Bu;

struct FrameArgs {
    const float2 *y;                            // [B][S]
    const float2 *gains;                        // [B][nh]
    const float2 *pilots;                       // [(J + 1) plen]
    int B, S, coh, nh, plen, dlen, J, T;
    uint64_t cw0, seed;
    float sigma;
    double cfo_max;
    float2 *frames, *h_true;                    // [B][T]; h_true nullable
};

// Position i of the flat [f.B][f.T] frames: row r = i / T holds codeword cw, its pilot noise drawn from
// pilot_domain
template <bool CFO>
__device__ __forceinline__ void frame_position(const FrameArgs &f, long i, long r, uint64_t cw, uint32_t pilot_domain) {
    const int t = (int)(i - r * f.T);
    const int t_last = f.S + f.J * f.plen;      // where pilot block J starts
    int j, off;
    if (t >= t_last) {
        j = f.J;
        off = t - t_last;
    } else {
        j = t / (f.plen + f.dlen);
        off = t - j * (f.plen + f.dlen);
    }
    float2 v, g;
    if (off < f.plen) {
        const int s = min(j * f.dlen, f.S - 1), k = j * f.plen + off;
        g = f.gains[r * f.nh + s / f.coh];
        const float2 p = f.pilots[k];
        const double hr = (double)g.x, hi = (double)g.y, pr = (double)p.x, pi = (double)p.y;
        const Philox4 q = philox4x32_10(Philox4{(uint32_t)cw, (uint32_t)(cw >> 32), (uint32_t)(k >> 1), pilot_domain},
                                        (uint32_t)f.seed, (uint32_t)(f.seed >> 32));
        const uint32_t a = (k & 1) ? q.z : q.x, b = (k & 1) ? q.w : q.y;
        const float u1 = ((float)(a >> 8) + 0.5f) * 0x1p-24f, u2 = ((float)(b >> 8) + 0.5f) * 0x1p-24f;
        const float rad = f.sigma * sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);
        v = make_float2((float)(hr * pr - hi * pi) + rad * cs, (float)(hr * pi + hi * pr) + rad * sn);
    } else {
        const int s = j * f.dlen + (off - f.plen);
        g = f.gains[r * f.nh + s / f.coh];
        v = f.y[r * f.S + s];
    }
    if constexpr (CFO) {
        const Philox4 q = philox4x32_10(Philox4{(uint32_t)cw, (uint32_t)(cw >> 32), 0u, CFO_DOMAIN}, (uint32_t)f.seed,
                                        (uint32_t)(f.seed >> 32));
        const double u = ((double)(q.x >> 8) + 0.5) * 0x1p-24;
        const double fg = f.cfo_max * (2.0 * u - 1.0);
        double sn, cs;
        sincospi(2.0 * (fg * (double)t), &sn, &cs);
        const double vr = (double)v.x, vi = (double)v.y, gr = (double)g.x, gi = (double)g.y;
        v = make_float2((float)(vr * cs - vi * sn), (float)(vr * sn + vi * cs));
        g = make_float2((float)(gr * cs - gi * sn), (float)(gr * sn + gi * cs));
    }
    f.frames[i] = v;
    if (f.h_true) f.h_true[i] = g;
}

template <bool CFO>
__global__ __launch_bounds__(BLOCK) void k_workload_frame(FrameArgs f) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (long)f.B * f.T) return;
    const long r = i / f.T;
    frame_position<CFO>(f, i, r, f.cw0 + (uint64_t)r, PILOT_DOMAIN);
}

// The same over R receive branches: f.B = codewords * R rows, row r branch r % R of
// codeword r / R, whose rotation all its branches share
template <bool CFO>
__global__ __launch_bounds__(BLOCK) void k_workload_frame_branches(FrameArgs f, int R) {
    const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (long)f.B * f.T) return;
    const long r = i / f.T;
    frame_position<CFO>(f, i, r, f.cw0 + (uint64_t)(r / R), PILOT_DOMAIN | (uint32_t)(r % R) << 16);
}

}  // namespace tdec
