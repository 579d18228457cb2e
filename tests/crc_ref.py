"""Bitwise / numpy restatement of the frame check.

TEST INFRASTRUCTURE (a plain module like harq_ref.py: numpy only, no GPU, nothing imported
from the package under test).  Restated from the issue's definitions, not from the library:

  A row is L bits, bit j its j-th element (only bit 0 of an element counts); the first L - r
  are payload, the last r the check field.  The bits go through the plain shift register in
  ascending j: MSB first, no reflection, no final XOR.

    kind     r   polynomial   initial register
    crc16    16  0x1021       0xFFFF            CRC-16/CCITT-FALSE
    crc32    32  0x04C11DB7   0xFFFFFFFF        CRC-32/MPEG-2

  register(bits, kind)      the register after the rows' bits, uint32 [B] (the serial loop,
                            vectorised over rows only)
  remainder(rows, kind)     register over all L bits: 0 iff the row passes
  attach(rows, kind)        a copy with the last r elements set to the register after the
                            first L - r, most significant bit first
  table(kind, L)            T[j] = x^(L-1-j) x^r mod g and the constant init x^L mod g: the
                            affine form, remainder = XOR of T[j] over set bits ^ constant
  remainder_affine(rows, kind)
  bytes_to_bits / g_bits    helpers for the pins and the designed rows
"""
import numpy as np

KINDS = {"crc16": (16, 0x1021, 0xFFFF), "crc32": (32, 0x04C11DB7, 0xFFFFFFFF)}


def _step(reg, bit, r, poly):
    """One register step for arrays of registers (Python ints or uint64) and bits."""
    mask = (1 << r) - 1
    top = (reg >> (r - 1)) & 1
    reg = (reg << 1) & mask
    return reg ^ (poly * (top ^ bit))


def register(bits, kind, init=None):
    """uint32 [B]: the register after bits [B][n] (any integer dtype, bit 0 of each), from the
    kind's initial value or `init`."""
    r, poly, init0 = KINDS[kind]
    b = (np.atleast_2d(np.asarray(bits)).astype(np.int64) & 1).astype(np.uint64)
    reg = np.full(b.shape[0], init0 if init is None else init, np.uint64)
    for j in range(b.shape[1]):
        reg = _step(reg, b[:, j], r, np.uint64(poly))
    return reg.astype(np.uint32)


def remainder(rows, kind):
    return register(rows, kind)


def check_field(reg, r):
    """[B][r] 0/1: the register's bits, most significant first."""
    reg = np.asarray(reg, np.uint64)
    return ((reg[:, None] >> np.arange(r - 1, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)


def attach(rows, kind):
    r = KINDS[kind][0]
    rows = np.atleast_2d(np.asarray(rows))
    out = rows.copy()
    out[:, -r:] = check_field(register(rows[:, :-r], kind), r).astype(rows.dtype)
    return out


def table(kind, L):
    """(T uint32 [L], constant): T[j] = x^(L-1-j) x^r mod g; constant = init x^L mod g."""
    r, poly, init = KINDS[kind]
    T = np.zeros(L, np.uint32)
    v = poly                                   # x^r mod g
    for j in range(L - 1, -1, -1):
        T[j] = v
        v = _step(v, 0, r, poly)
    c = init
    for _ in range(L):
        c = _step(c, 0, r, poly)
    return T, np.uint32(c)


def remainder_affine(rows, kind):
    rows = np.atleast_2d(np.asarray(rows))
    T, c = table(kind, rows.shape[1])
    sel = (rows.astype(np.int64) & 1).astype(bool)
    return np.bitwise_xor.reduce(np.where(sel, T[None, :], np.uint32(0)), axis=1) ^ c


def bytes_to_bits(data):
    """Bit j of the row is bit 7 - j % 8 of byte j / 8."""
    return np.unpackbits(np.frombuffer(bytes(data), np.uint8)).astype(np.uint8)


def g_bits(kind):
    """g(x) as r + 1 bits, x^r first."""
    r, poly, _ = KINDS[kind]
    return np.array([1] + [(poly >> (r - 1 - i)) & 1 for i in range(r)], np.uint8)
