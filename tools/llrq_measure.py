#!/usr/bin/env python3
"""Cost of the quantised LLR paths, in one process, interleaved round by round
in both orders (round 0 untimed):

  depuncture  llrq_depuncture_dev on int8 and float16 rows against tdec_depuncture_dev on float32
              rows, HIP events around each launch.  The float32 rows are the widened int8 rows, so
              the two write the same planes, which is checked.
  host        llrq_decode_batch on int8 host rows against tdec_decode_batch on the widened float32
              rows, from page-locked and from pageable numpy buffers, the host clock around each
              (synchronous) call, in codewords/s.  The bits are checked to be the same.

  python tools/llrq_measure.py [--batch 1048576 --host-batch 262144 --rounds 5] [--out f.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402

STEP = np.float32(30 / 127)


def stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}


def depuncture(a, dev):
    codec = M.DVBRCS2_Turbo(a.n, a.rate, interleaver="valid-perm", device=0)
    B, L = a.batch, codec.handle.llr_len
    rows = {"int8": torch.randint(-127, 128, (B, L), dtype=torch.int8, device=dev)}
    rows["f32"] = rows["int8"].to(torch.float32) * float(STEP)            # one f32 multiply, as the kernel's
    rows["f16"] = (torch.randn((B, L), dtype=torch.float32, device=dev) * 8).to(torch.float16)
    planes = torch.empty(codec.planes_bytes(B) // 4, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream()
    kinds = ["f32", "int8", "f16"]
    times, sums = {k: [] for k in kinds}, {}
    for r in range(2 * a.rounds + 1):                  # round 0 untimed; odd rounds forward, even rounds reversed
        for k in (kinds if r % 2 else kinds[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            codec.depuncture_device(rows[k], planes, llr_step=STEP if k == "int8" else None)
            e1.record(st)
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1))
            else:
                sums[k] = planes.view(torch.int32).sum(dtype=torch.int64).item()
    assert sums["f32"] == sums["int8"], "int8 planes differ from the float32 kernel's"
    ms = {k: stats(t) for k, t in times.items()}
    spread = ms["f32"]["max"] - ms["f32"]["min"]
    plane_b = codec.planes_bytes(B)
    return {"what": "depuncture", "n_couples": a.n, "rate": a.rate, "codewords": B, "llr_len": int(L),
            "rounds_each_order": a.rounds, "ms": ms, "f32_spread_ms": spread,
            "bytes": {"f32": 4 * B * L + plane_b, "f16": 2 * B * L + plane_b, "int8": B * L + plane_b},
            "within_f32_spread": {k: ms[k]["median"] <= ms["f32"]["median"] + spread for k in ("int8", "f16")}}


def host(a):
    codec = M.DVBRCS2_Turbo(a.n, a.rate, interleaver="valid-perm", device=0)
    B, L = a.host_batch, codec.handle.llr_len
    rng = np.random.default_rng(7)
    q = rng.integers(-127, 128, (B, L), dtype=np.int8)
    bufs = {}
    for mem in ("pinned", "pageable"):
        alloc = codec.host_buffer if mem == "pinned" else np.empty
        bufs[mem, "int8"], bufs[mem, "f32"] = alloc((B, L), np.int8), alloc((B, L), np.float32)
        bufs[mem, "int8"][...] = q
        np.multiply(q, STEP, out=bufs[mem, "f32"], dtype=np.float32)
        bufs[mem, "out"] = alloc((B, codec.k_info), np.int32)
    variants = [(mem, k) for mem in ("pinned", "pageable") for k in ("f32", "int8")]
    times, sums = {v: [] for v in variants}, {}
    for r in range(2 * a.rounds + 1):
        for mem, k in (variants if r % 2 else variants[::-1]):
            t0 = time.perf_counter()
            codec.decode_batch(bufs[mem, k], out=bufs[mem, "out"], llr_step=STEP if k == "int8" else None)
            dt = time.perf_counter() - t0
            if r:
                times[mem, k].append(B / dt)
            else:
                sums[mem, k] = int(bufs[mem, "out"].sum(dtype=np.int64))
    assert len(set(sums.values())) == 1, "the int8 and float32 host paths decode different bits"
    cps = {f"{mem} {k}": stats(t) for (mem, k), t in times.items()}
    out_b = 4 * codec.k_info
    rec = {"what": "host", "n_couples": a.n, "rate": a.rate, "codewords": B, "rounds_each_order": a.rounds,
           "codewords_per_s": cps, "bytes_per_codeword": {"f32": 4 * L + out_b, "int8": L + out_b},
           "byte_ratio_f32_over_int8": (4 * L + out_b) / (L + out_b), "ratio_int8_over_f32": {}, "within_f32_spread": {}}
    for mem in ("pinned", "pageable"):
        f, i = cps[f"{mem} f32"], cps[f"{mem} int8"]
        rec["ratio_int8_over_f32"][mem] = i["median"] / f["median"]
        rec["within_f32_spread"][mem] = i["median"] >= f["median"] - (f["max"] - f["min"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=752)
    ap.add_argument("--rate", default="1/3")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--host-batch", type=int, default=1 << 18)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    recs = []
    for rec in (depuncture(a, dev), None):
        if rec is None:
            torch.cuda.empty_cache()
            rec = host(a)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
