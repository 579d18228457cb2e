#!/usr/bin/env python3
"""Cost of the maximal-ratio combiner, in one process with HIP events, both
orders, on the branch generator's symbols: tdec_combine_dev with R = 1, 2, 4 branches, common
(scalar) and per-branch noise, coh = 1 and coh = S, against tdec_equalize_dev on the same
shapes (one branch) as the yardstick.  R = 1 with common noise writes what the equaliser
writes, which is checked.  Bytes are the algorithmic ones per combined symbol: 8 R in for y,
8 R / coh in for h, 16 out (the equaliser: R = 1).

  python tools/diversity_measure.py [--mods 16QAM 256QAM --batch 1048576 --rounds 5] [--out f.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from modulations_amd import demap as D  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402
from modulations_amd.workload import make_symbols  # noqa: E402


def stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}


def measure(mod, coh_burst, a, dev):
    codec = M.DVBRCS2_Turbo(a.n, a.rate, interleaver="valid-perm", device=0)
    B = a.batch
    S = -(-codec.handle.enc_len // D.MODULATIONS[mod]["bps"])
    coh = S if coh_burst else 1
    z, nvs = torch.empty((B, S), dtype=torch.complex64, device=dev), torch.empty((B, S), dtype=torch.float64, device=dev)
    z1, nvs1 = torch.empty_like(z), torch.empty_like(nvs)
    st = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    data, variants, by = {}, [], {}
    n0 = None
    for R in a.branches:
        _, y, n0, h = make_symbols(codec, B, mod, a.ebn0, 99, dev, want_info=False,
                                   fading={"K": 0.0, "coh": coh, "branches": R})
        nvb = torch.full((B, R), float(n0), dtype=torch.float64, device=dev)
        data[R] = (y, h, nvb)
        per_sym = 8.0 * R + 8.0 * R / coh + 16.0
        variants.append((f"combine R={R}", lambda d=data[R]: D.combine_device(d[0], d[1], n0, coh=coh, out=z, nv_out=nvs)))
        variants.append((f"combine R={R}, per-branch noise",
                         lambda d=data[R]: D.combine_device(d[0], d[1], d[2], coh=coh, out=z, nv_out=nvs)))
        by[f"combine R={R}"] = by[f"combine R={R}, per-branch noise"] = per_sym * B * S
    y0, h0 = data[a.branches[0]][0][:, 0].contiguous(), data[a.branches[0]][1][:, 0].contiguous()
    variants.append(("equaliser", lambda: D.equalize_device(y0, h0, n0, coh=coh, out=z1, nv_out=nvs1)))
    by["equaliser"] = (8.0 + 8.0 / coh + 16.0) * B * S
    times = {k: [] for k, _ in variants}
    for r in range(2 * a.rounds + 1):                  # round 0 untimed; odd rounds forward, even rounds reversed
        for k, fn in (variants if r % 2 else variants[::-1]):
            t = timed(fn)
            if r:
                times[k].append(t)
    same = None
    if a.branches[0] == 1:
        variants[0][1]()
        variants[-1][1]()
        torch.cuda.synchronize()
        same = bool(torch.equal(z.view(torch.int64), z1.view(torch.int64)) and
                    torch.equal(nvs.view(torch.int64), nvs1.view(torch.int64)))
        assert same, f"{mod}: R = 1 combine and the equaliser differ"
    ms = {k: stats(t) for k, t in times.items()}
    rec = {"mod": mod, "n_couples": a.n, "rate": a.rate, "codewords": B, "symbols": S, "coh": coh,
           "ebn0_db": a.ebn0, "rounds_each_order": a.rounds, "one_branch_equals_equaliser": same, "ms": ms, "bytes": by,
           "tb_per_s": {k: by[k] / (ms[k]["median"] * 1e-3) / 1e12 for k in ms},
           "over_equaliser": {k: ms[k]["median"] / ms["equaliser"]["median"] for k in ms}}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mods", nargs="+", default=["16QAM", "256QAM"])
    ap.add_argument("--branches", nargs="+", type=int, default=[1, 2, 4])
    ap.add_argument("--n", type=int, default=752)
    ap.add_argument("--rate", default="1/3")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ebn0", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    recs = []
    for m in a.mods:
        for coh_burst in (False, True):
            recs.append(measure(m, coh_burst, a, dev))
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
