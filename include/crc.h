/* crc.h -- frame check on the device: CRC attach and verify over rows
 * of 0/1 elements, and the workload generator fed with the caller's info bits.
 *
 * Built into libtdec.so beside include/tdec.h and include/harq.h, whose conventions hold:
 * device pointers, stream-ordered, 0 or a negative TDEC_E* code with the reason in the
 * library's thread-local last-error string (tdec_last_error), an empty batch a no-op before
 * the pointers are looked at.
 *
 * A row is row_bits elements, one bit each: of an element wider than one bit only bit 0 is
 * looked at.  Bit j of a row is its j-th element (info-bit order A0 B0 A1 B1 ..., as
 * tdec_info_bits_dev and the decoders write it).  The first row_bits - r bits are payload,
 * the last r the check field.  The bits go through the plain shift register in ascending j:
 * MSB first, no reflection, no final XOR (viewed as bytes, bit j is bit 7 - j % 8 of byte
 * j / 8).
 *
 *   kind        r   polynomial   initial register   catalogue name
 *   CRC_KIND16  16  0x1021       0xFFFF             CRC-16/CCITT-FALSE
 *   CRC_KIND32  32  0x04C11DB7   0xFFFFFFFF         CRC-32/MPEG-2
 *
 * The check field holds the register after the payload, most significant bit first; the
 * register over all row_bits bits of a valid row, the remainder, is therefore 0, and a row
 * passes iff its remainder is 0.
 *
 * The kernels read a table of row_bits words that depends on (kind, row_bits) only.  It is
 * built on the host and uploaded at the first call for a (device, kind, row_bits): that call
 * allocates and synchronises, and is refused (TDEC_EUNSUPPORTED) on a stream that is being
 * captured.  Every later call for the triple is allocation free and synchronisation free.
 * Rows are read with vector loads where the base pointer allows (16-byte aligned int32 rows,
 * 8-byte aligned uint8 rows) and element by element otherwise.
 *
 * TDEC_EINVAL: unknown kind, row_bits % 8 != 0, row_bits <= r, row_bits > CRC_MAX_ROW_BITS,
 * negative B, a null pointer (d_rem excepted) with B > 0.
 */
#ifndef CRC_H
#define CRC_H

#include "tdec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRC_KIND16 16
#define CRC_KIND32 32
#define CRC_MAX_ROW_BITS 2048
/* The launch: blocks of CRC_ROWS_PER_BLOCK waves, one row per wave at a time, at most
 * CRC_MAX_BLOCKS blocks; rows beyond CRC_MAX_BLOCKS * CRC_ROWS_PER_BLOCK are reached by a
 * grid-stride loop. */
#define CRC_ROWS_PER_BLOCK 4
#define CRC_MAX_BLOCKS 2048

/* Overwrites the last r elements of each uint8 [B][row_bits] row with the check field of its
 * first row_bits - r elements, as 0/1 bytes.  The payload is not written. */
int crc_attach_dev(int device, int kind, long B, int row_bits, uint8_t *d_rows_u8, void *stream);

/* d_ok[b] = 1 if row b's remainder is 0, else 0 (int32 [B]); d_rem (nullable, uint32 [B])
 * receives the remainder.  Rows of int32 elements (the decoders' output). */
int crc_check_dev(int device, int kind, long B, int row_bits, const int32_t *d_bits_i32, int32_t *d_ok,
                  uint32_t *d_rem, void *stream);

/* crc_check_dev over rows of uint8 elements (the generators' info bytes). */
int crc_check_u8_dev(int device, int kind, long B, int row_bits, const uint8_t *d_bits_u8, int32_t *d_ok,
                     uint32_t *d_rem, void *stream);

/* harq_workload_tx_dev (include/harq.h) with the caller's info bits, uint8 [B][2N] 0/1
 * bytes at an 8-byte aligned d_bits_in, in place of the counter-based ones: the same encoder,
 * mapping, noise and gains of (seed, cw0 + c, tx), so that bits which equal the counter-based
 * ones give harq_workload_tx_dev's symbols and gains bit for bit.  Its refusals, and
 * TDEC_EINVAL for a null d_bits_in. */
int crc_workload_tx_dev(tdec_t *h, int B, int tx, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                        double sigma, int fading, double rician_k, int coh, const uint8_t *d_bits_in, float *d_syms,
                        float *d_h, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRC_H */
