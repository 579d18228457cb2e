// tdec_crc.hip -- frame check (include/crc.h): the CRC of rows of 0/1
// elements as a data-parallel reduction.
//
// The shift register is affine over GF(2).  After n bits b_0 .. b_(n-1), with r the width,
// g the polynomial and init the initial register,
//   reg = init x^n + sum_j b_j x^(n-1-j) x^r   (mod g)
// so a row's register is the XOR, over its set bits j, of one table word, XORed with one
// constant.  With T[j] = x^(L-1-j) x^r mod g for a row of L bits:
//   verify (n = L)      remainder   = XOR T[j]     ^ init x^L     mod g
//   attach (n = L - r)  check field = XOR T[j + r] ^ init x^(L-r) mod g
// one table of L words per (kind, L) serves both; the two constants come by value.
//
// Layout: blocks of CRC_WAVES waves.  A block stages the table in LDS once (8 KB at the
// longest row), then each wave takes one row at a time in a grid-stride loop with no further
// barrier: a lane loads VB bytes per sweep (16 of int32 elements, 8 of uint8 ones), all of a
// row's sweeps before their use, XORs the table words of its set bits (LDS reads of 16 B,
// consecutive lanes consecutive addresses) and the wave reduces with shuffles.  Row lengths
// are multiples of 8 elements, so a row is whole vectors; a base pointer that is not aligned
// to VB takes element loads instead.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tdec {

constexpr int CRC_WAVES = 4;                    // rows a block works on at a time (CRC_ROWS_PER_BLOCK)
constexpr int CRC_MAX_L = 2048;                 // CRC_MAX_ROW_BITS

struct CrcArgs {
    const void *in;                             // [B][L] elements, bit 0 of each
    void *out;                                  // attach: the same rows, written at [L - r, L)
    long B;
    int L, r;
    uint32_t c0;                                // init x^n mod g
    const uint32_t *table;                      // T[L], 16-byte aligned
    int32_t *ok;                                // verify: [B]
    uint32_t *rem;                              // verify: [B] (nullable)
    int vec;                                    // `in` is aligned to the vector width
};

// XOR of tab[j0 .. j0 + 3] under bits 0 of four elements
__device__ __forceinline__ uint32_t crc_take4(const uint4 t, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    return (t.x & (0u - (b0 & 1u))) ^ (t.y & (0u - (b1 & 1u))) ^ (t.z & (0u - (b2 & 1u))) ^ (t.w & (0u - (b3 & 1u)));
}

// E: int32_t (lanes load int4, 4 elements) or uint8_t (uint2, 8 elements).  ATTACH: the
// register over the first L - r elements written as r 0/1 elements behind them; else the
// register over all L to ok / rem.
template <typename E, bool ATTACH>
__global__ __launch_bounds__(CRC_WAVES * 64) void k_crc(CrcArgs a) {
    constexpr int EPL = sizeof(E) == 4 ? 4 : 8;             // elements per lane per sweep
    constexpr int SWEEPS = CRC_MAX_L / (64 * EPL);          // of the longest row
    __shared__ uint4 tab4[CRC_MAX_L / 4];
    const uint32_t *tab = reinterpret_cast<const uint32_t *>(tab4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < a.L / 4; i += CRC_WAVES * 64) tab4[i] = reinterpret_cast<const uint4 *>(a.table)[i];
    __syncthreads();
    const int n = ATTACH ? a.L - a.r : a.L;                 // elements read, a multiple of 8
    const int off = ATTACH ? a.r : 0;                       // table word of element 0, a multiple of 4
    const int nv = n / EPL;
    for (long row = (long)blockIdx.x * CRC_WAVES + wave; row < a.B; row += (long)gridDim.x * CRC_WAVES) {
        const E *p = static_cast<const E *>(a.in) + row * a.L;
        uint32_t acc = 0;
        if (a.vec) {
            if constexpr (sizeof(E) == 4) {
                int4 v[SWEEPS];
#pragma unroll
                for (int s = 0; s < SWEEPS; ++s) {
                    const int i = lane + 64 * s;
                    v[s] = i < nv ? reinterpret_cast<const int4 *>(p)[i] : make_int4(0, 0, 0, 0);
                }
#pragma unroll
                for (int s = 0; s < SWEEPS; ++s) {
                    const int i = lane + 64 * s;
                    if (i < nv) acc ^= crc_take4(tab4[i + off / 4], v[s].x, v[s].y, v[s].z, v[s].w);
                }
            } else {
                uint2 v[SWEEPS];
#pragma unroll
                for (int s = 0; s < SWEEPS; ++s) {
                    const int i = lane + 64 * s;
                    v[s] = i < nv ? reinterpret_cast<const uint2 *>(p)[i] : make_uint2(0, 0);
                }
#pragma unroll
                for (int s = 0; s < SWEEPS; ++s) {
                    const int i = lane + 64 * s;
                    if (i < nv) {
                        const uint32_t x = v[s].x, y = v[s].y;
                        acc ^= crc_take4(tab4[2 * i + off / 4], x, x >> 8, x >> 16, x >> 24);
                        acc ^= crc_take4(tab4[2 * i + 1 + off / 4], y, y >> 8, y >> 16, y >> 24);
                    }
                }
            }
        } else {
            for (int j = lane; j < n; j += 64) acc ^= tab[j + off] & (0u - ((uint32_t)p[j] & 1u));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc ^= __shfl_xor(acc, o);
        const uint32_t reg = acc ^ a.c0;
        if constexpr (ATTACH) {
            if (lane < a.r) static_cast<E *>(a.out)[row * a.L + n + lane] = (E)((reg >> (a.r - 1 - lane)) & 1u);
        } else if (lane == 0) {
            a.ok[row] = reg == 0;
            if (a.rem) a.rem[row] = reg;
        }
    }
}

}  // namespace tdec
