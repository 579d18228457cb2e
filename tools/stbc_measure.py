#!/usr/bin/env python3
"""Cost of the Alamouti combiner, in one process with HIP events, both orders, on
the generators' symbols: stbc_combine_dev with R = 1, 2, 4 receive branches and common (scalar)
noise, coh = 2 and coh = S2, against tdec_combine_dev of the same R on the same shapes (the
maximal-ratio combiner: the same y bytes per symbol, half the gains) as the yardstick.  Bytes are
the algorithmic ones per combined symbol: 8 R in for y, 16 R / coh in for h (the yardstick: 8 R /
coh), 16 out.

  python tools/stbc_measure.py [--mods 16QAM --batch 1048576 --rounds 5] [--out f.json]"""
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
    S2 = S + (S & 1)
    coh = S2 if coh_burst else 2
    z, nvs = torch.empty((B, S), dtype=torch.complex64, device=dev), torch.empty((B, S), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    variants, by, times = [], {}, {}
    n0 = None
    for R in a.branches:                               # one R at a time: R = 4 holds 2 x 4 x B x S2 complex64
        fading = {"K": 0.0, "coh": coh, "branches": R}
        _, y2, n0, h2 = make_symbols(codec, B, mod, a.ebn0, 99, dev, want_info=False, fading={**fading, "tx_antennas": 2})
        _, y1, _, h1 = make_symbols(codec, B, mod, a.ebn0, 99, dev, want_info=False, fading=fading)
        variants = [(f"stbc R={R}", lambda: D.stbc_combine_device(y2, h2, n0, S=S, coh=coh, out=z, nv_out=nvs)),
                    (f"mrc R={R}", lambda: D.combine_device(y1, h1, n0, coh=coh, out=z, nv_out=nvs))]
        by[f"stbc R={R}"] = (8.0 * R * S2 / S + 16.0 * R / coh + 16.0) * B * S
        by[f"mrc R={R}"] = (8.0 * R + 8.0 * R / coh + 16.0) * B * S
        for k, _ in variants:
            times[k] = []
        for r in range(2 * a.rounds + 1):              # round 0 untimed; odd rounds forward, even rounds reversed
            for k, fn in (variants if r % 2 else variants[::-1]):
                t = timed(fn)
                if r:
                    times[k].append(t)
        del y1, y2, h1, h2
        torch.cuda.empty_cache()
    ms = {k: stats(t) for k, t in times.items()}
    rec = {"mod": mod, "n_couples": a.n, "rate": a.rate, "codewords": B, "symbols": S, "slots": S2, "coh": coh,
           "ebn0_db": a.ebn0, "rounds_each_order": a.rounds, "ms": ms, "bytes": by,
           "tb_per_s": {k: by[k] / (ms[k]["median"] * 1e-3) / 1e12 for k in ms},
           "over_mrc": {f"R={R}": ms[f"stbc R={R}"]["median"] / ms[f"mrc R={R}"]["median"] for R in a.branches}}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mods", nargs="+", default=["16QAM"])
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
