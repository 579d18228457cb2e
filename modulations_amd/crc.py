"""Frame check on the device (include/crc.h): a CRC attached to the
info bits of a codeword and verified on the decoder's output, so that a receiver can tell a
wrong decode without knowing the transmitted bits.

A row is L bits, one per element (bit 0 of it), in info-bit order A0 B0 A1 B1 ...; the first
L - r are payload, the last r the check field, the shift register's value after the payload,
most significant bit first.  MSB first, no reflection, no final XOR:

  "crc16"  r = 16  polynomial 0x1021      initial 0xFFFF       (CRC-16/CCITT-FALSE)
  "crc32"  r = 32  polynomial 0x04C11DB7  initial 0xFFFFFFFF   (CRC-32/MPEG-2)

The register over all L bits of a valid row, the remainder, is 0: a row passes iff it is.
The first call for a (device, kind, L) uploads a table and synchronises; later calls are
stream-ordered and allocation free."""
from __future__ import annotations

from . import _native as _n

KINDS = {"crc16": {"r": 16, "poly": 0x1021, "init": 0xFFFF},
         "crc32": {"r": 32, "poly": 0x04C11DB7, "init": 0xFFFFFFFF}}
MAX_ROW_BITS = 2048
# rows one trip of the launch's grid covers (CRC_MAX_BLOCKS * CRC_ROWS_PER_BLOCK of include/crc.h);
# a larger batch takes the kernel's grid-stride loop
GRID_ROWS = 2048 * 4


def _kind(kind):
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError(f"unknown CRC kind {kind!r} ({', '.join(KINDS)})")
    return _n.CRC_KINDS[kind]


def payload_bits(codec, kind):
    """Info bits of a codeword of `codec` that are left for the payload."""
    n = codec.k_info - _kind(kind)
    if n <= 0:
        raise ValueError(f"{kind} does not fit the {codec.k_info} info bits of N = {codec.N}")
    return n


def _rows(t, name, dtypes):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise TypeError(f"{name} must be a tensor of {' or '.join(str(d) for d in dtypes)}")
    if t.dim() != 2 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [B, L] tensor on a HIP device")
    return t.shape


def _stream(t, stream):
    import torch
    return _n.stream_ptr(stream) if stream is not None else torch.cuda.current_stream(t.device).cuda_stream


def attach_device(info, kind, stream=None):
    """Overwrite the last r bytes of each row of `info` (uint8 [B, L] of 0/1 on the device)
    with the check field of the first L - r; the payload is not written.  Returns `info`."""
    import torch
    k = _kind(kind)
    B, L = _rows(info, "info", (torch.uint8,))
    _n.check(_n.lib().crc_attach_dev(info.device.index, k, B, L, _n.ptr(info), _stream(info, stream)))
    return info


def check_device(bits, kind, ok=None, rem=None, stream=None):
    """ok int32 [B]: 1 where the row of `bits` (int32 or uint8 [B, L] on the device, bit 0 of
    each element) leaves remainder 0, else 0.  ok: the tensor to fill (None: a new one).  rem
    (optional): an int32 [B] tensor that receives the remainder's 32 bits (view it as
    unsigned, `rem.cpu().numpy().view("uint32")`).  Returns ok."""
    import torch
    k = _kind(kind)
    B, L = _rows(bits, "bits", (torch.int32, torch.uint8))
    if ok is None:
        ok = torch.empty(B, dtype=torch.int32, device=bits.device)
    for t, name in ((ok, "ok"), (rem, "rem")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (B,)
                              or t.device != bits.device or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 [{B}] tensor on the bits' device")
    fn = _n.lib().crc_check_dev if bits.dtype == torch.int32 else _n.lib().crc_check_u8_dev
    _n.check(fn(bits.device.index, k, B, L, _n.ptr(bits), _n.ptr(ok), _n.ptr(rem), _stream(bits, stream)))
    return ok
