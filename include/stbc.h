/* stbc.h -- transmit diversity: the Alamouti space-time block code
 * over two transmit antennas and R receive branches, its linear combiner and the
 * counter-based workload generator's 2 x R link.
 *
 * Built into libtdec.so beside include/tdec.h, whose conventions hold: device pointers,
 * stream-ordered and allocation free, 0 or a negative TDEC_E* code with the reason in the
 * library's thread-local last-error string, an empty batch a no-op before the pointers
 * are looked at.
 *
 * The code.  A codeword's S table points are x[0 .. S-1]; S2 = S + (S & 1), and for an odd
 * S the pad point is x[S] = 0 + 0j.  Pair m is (x[2m], x[2m+1]), sent in two slots:
 *
 *     slot 2m      antenna 0:  x[2m]             antenna 1:  x[2m+1]
 *     slot 2m+1    antenna 0: -conj(x[2m+1])     antenna 1:  conj(x[2m])
 *
 * Receive branch r sees y = h0 s0 + h1 s1 + n in each slot, h0 and h1 the EFFECTIVE gains
 * of its two paths: the split of the transmit power between the antennas is inside the
 * gains (the generator writes gains with E|h_a|^2 = 1/2), and the combiner holds no
 * sqrt(2).  A gain block covers coh slots; coh is even, so a pair never straddles blocks.
 *
 * The combiner, all in f64 without contraction, the branches in the order r = 0 .. R-1.
 * With y0 = y[2m], y1 = y[2m+1] of branch r and (h0, h1) its gains of block 2m / coh,
 * every f32 component widened to f64 first (each product below is then exact):
 *
 *     g_r      = (h0r*h0r + h0i*h0i) + (h1r*h1r + h1i*h1i)
 *     num0_r   = conj(h0) y0 + h1 conj(y1)                        (the even symbol)
 *       .re    = (y0r*h0r + y0i*h0i) + (y1r*h1r + y1i*h1i)
 *       .im    = (y0i*h0r - y0r*h0i) + (y1r*h1i - y1i*h1r)
 *     num1_r   = conj(h1) y0 - h0 conj(y1)                        (the odd symbol)
 *       .re    = (y0r*h1r + y0i*h1i) - (y1r*h0r + y1i*h0i)
 *       .im    = (y0i*h1r - y0r*h1i) - (y1r*h0i - y1i*h0r)
 *
 * the three additions of each part in the order the brackets give: the two inner ones,
 * then the outer one.  (With h1 = 0 the even symbol's terms are the equaliser's,
 * include/tdec.h's tdec_equalize_dev.)
 *
 * A branch whose g_r is zero or not finite is skipped.  Common noise (the scalar
 * noise_var, or d_nv_rows[b]): G, N0, N1 are the sums of g_r, num0_r, num1_r over the live
 * branches, each sum starting from the first live branch's term, not from 0.0, and
 *
 *     z[2m] = (float)(N0 / G)   z[2m+1] = (float)(N1 / G)   nv_sym[2m] = nv_sym[2m+1] = nv_b / G
 *
 * Per-branch noise (d_nv_branches[b][r]): the summed terms are g_r / nv_br, num0_r / nv_br
 * and num1_r / nv_br (each component divided), z likewise, nv_sym = 1.0 / G: what
 * tdec_combine_dev does.  No live branch, or a G that came out zero or infinite: an
 * erasure, z = 0 and nv_sym = +inf.  A NaN nv_br makes G NaN in every pair of its row that
 * the branch is live in, and nothing else; a NaN y makes its own pair NaN, and nothing
 * else.  No floor here: the demapper floors.
 */
#ifndef STBC_H
#define STBC_H

#include "tdec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* d_y complex64 [B][R][S2], d_h complex64 [B][R][2][nh] with nh = ceil(S2 / coh) (antenna a
 * of branch r at [b][r][a]), 1 <= R <= 8 -> d_z complex64 [B][S], d_nv_sym f64 [B][S], the
 * shape tdec_equalize_dev and tdec_combine_dev write.  For an odd S the pad slot's second
 * output does not exist and is not written.  Noise: noise_var, or d_nv_rows f64 [B], or
 * d_nv_branches f64 [B][R]; one array at most.
 * A pair's y is one 16-byte load where d_y is 16-byte aligned (S2 is even: every branch
 * row then is); z and nv_sym are written 16 bytes at a time where S is even and both are
 * 16-byte aligned, else 8 bytes at a time.
 * B == 0 or S == 0: a no-op.  TDEC_EINVAL, and nothing written: a null d_y, d_h, d_z or
 * d_nv_sym, a negative B or S, coh < 2 or odd, R outside 1 .. 8, both noise arrays. */
int stbc_combine_dev(int device, const float *d_y, const float *d_h, int B, int R, int S, int coh, double noise_var,
                     const double *d_nv_rows, const double *d_nv_branches, float *d_z, double *d_nv_sym, void *stream);

/* The 2 x R link of global codewords cw0 .. cw0 + B - 1: the info bits of (seed, cw0 + c)
 * and their labels as in every generator call, shared by the branches, sent as above.
 * d_syms complex64 [B][R][S2], d_h complex64 [B][R][2][nh], nh = ceil(S2 / coh), coh even.
 * Raw gain of antenna 0 to branch b, block j: the branch generator's draw (domain word
 * 0x3C5D | b << 16); of antenna 1: the same draw on the domain word 0x6F8A | b << 16.  The
 * written, effective gain is the raw one times 0.70710678118654752f per component in f32.
 * Slot s of branch b, (s0, s1) what the two antennas send in it, all f32, no contraction:
 *     re = ((h0r*s0r - h0i*s0i) + (h1r*s1r - h1i*s1i)) + n.re
 *     im = ((h0r*s0i + h0i*s0r) + (h1r*s1i + h1i*s1r)) + n.im
 * n the sample tdec_workload_branches_dev adds at symbol s of branch b (domain word
 * 0x2B0E | b << 16); the pad slot of an odd S draws its own at s = S.  A codeword depends
 * on its global index only.  d_info (nullable) receives the info bits.
 * TDEC_EINVAL: as tdec_workload_branches_dev, and coh < 2 or odd. */
int stbc_workload_dev(tdec_t *h, int B, int R, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                      double sigma, double rician_k, int coh, float *d_syms, float *d_h, uint8_t *d_info, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STBC_H */
