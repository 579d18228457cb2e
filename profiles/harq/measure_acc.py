"""Cost of harq_depuncture_acc_dev against tdec_depuncture_dev: HIP events, both orders, one process."""
import json
import sys

import torch

from modulations_amd import dvb_rcs2_turbo as M

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1048576
N = 752
c = M.DVBRCS2_Turbo(N, "1/3")
walk = c.handle.llr_len
planes = torch.zeros(c.planes_bytes(B) // 4, dtype=torch.float32, device="cuda")
llr = torch.randn((B, walk), dtype=torch.float32, device="cuda")
half = torch.where(torch.rand(B, device="cuda") < 0.5, torch.arange(B, dtype=torch.int32, device="cuda"),
                   torch.full((B,), -1, dtype=torch.int32, device="cuda"))
ident = torch.arange(B, dtype=torch.int32, device="cuda")
selected = int((half >= 0).sum())
calls = {"depuncture": lambda: c.depuncture_device(llr, planes),
         "acc_all": lambda: c.depuncture_accumulate_device(llr, planes, B),
         "acc_all_row_of": lambda: c.depuncture_accumulate_device(llr, planes, B, row_of=ident),
         "acc_half": lambda: c.depuncture_accumulate_device(llr, planes, B, row_of=half)}
step = N * B
bytes_of = {"depuncture": 48 * step, "acc_all": 72 * step, "acc_all_row_of": 72 * step + 4 * step,
            "acc_half": 72 * N * selected + 4 * step}
for f in calls.values():
    f()
torch.cuda.synchronize()
ms = {k: [] for k in calls}
for order in (list(calls), list(calls)[::-1]) * 3:
    for k in order:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        calls[k]()
        b.record()
        b.synchronize()
        ms[k].append(a.elapsed_time(b))
out = {"B": B, "N": N, "rate": "1/3", "selected_in_half": selected, "ms": ms,
       "median_ms": {k: sorted(v)[len(v) // 2] for k, v in ms.items()},
       "bytes": bytes_of}
out["TBps"] = {k: bytes_of[k] / (out["median_ms"][k] * 1e-3) / 1e12 for k in calls}
out["ratio_acc_all_over_depuncture"] = out["median_ms"]["acc_all"] / out["median_ms"]["depuncture"]
print(json.dumps(out))
