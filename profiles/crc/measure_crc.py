"""Throughput of crc_check_dev against tdec_count_errors_dev on the same bits: HIP events, both
orders, three times each, one process.  Run from the repository root with it on PYTHONPATH."""
import json
import sys

import torch

from modulations_amd import crc as CRC
from modulations_amd import dvb_rcs2_turbo as M
from modulations_amd import workload as W

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1048576
N, SEED = 752, 7
c = M.DVBRCS2_Turbo(N, "1/3")
L = c.k_info
info = W.info_bits(c, B, SEED, "cuda")
bits = info.to(torch.int32)                        # the decoders' element type; equal to the counter-based bits
valid = CRC.attach_device(info.clone(), "crc16").to(torch.int32)
ok = torch.empty(B, dtype=torch.int32, device="cuda")
rem = torch.empty(B, dtype=torch.int32, device="cuda")
calls = {"count_errors": lambda: W.count_errors(c, bits, SEED),
         "crc16_check": lambda: CRC.check_device(bits, "crc16", ok=ok),
         "crc32_check": lambda: CRC.check_device(bits, "crc32", ok=ok),
         "crc16_check_rem": lambda: CRC.check_device(valid, "crc16", ok=ok, rem=rem),
         "crc16_check_u8": lambda: CRC.check_device(info, "crc16", ok=ok),
         "crc16_attach_u8": lambda: CRC.attach_device(info, "crc16")}
row = {k: 4 * L for k in calls}
row["crc16_check_u8"], row["crc16_attach_u8"] = L, L - 16
for f in calls.values():
    f()
torch.cuda.synchronize()
assert int(W.count_errors(c, bits, SEED).sum()) == 0 and bool(CRC.check_device(valid, "crc16").all())
ms = {k: [] for k in calls}
for order in (list(calls), list(calls)[::-1]) * 3:
    for k in order:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        calls[k]()
        b.record()
        b.synchronize()
        ms[k].append(a.elapsed_time(b))
out = {"B": B, "N": N, "row_bits": L, "ms": ms, "median_ms": {k: sorted(v)[len(v) // 2] for k, v in ms.items()},
       "bytes_read_per_row": row}
out["TBps"] = {k: row[k] * B / (out["median_ms"][k] * 1e-3) / 1e12 for k in calls}
out["ratio_crc16_check_over_count_errors"] = out["median_ms"]["crc16_check"] / out["median_ms"]["count_errors"]
print(json.dumps(out))
