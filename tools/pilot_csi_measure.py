#!/usr/bin/env python3
"""Cost of the pilot-aided estimator, in one process with HIP events, both
orders, on framed bursts of the fading generator:
  (a) fused      tdec_csi_pilots_dev: estimate + interpolate + strip + equalise, one launch
  (b) unfused    tdec_csi_strip_dev, then tdec_equalize_dev on its y and h (coh = 1)
  (c) equaliser  tdec_equalize_dev alone on known per-symbol gains (the path without pilots)
(a) and (b) write the same z and nv_sym, which is checked.  Bytes are the algorithmic ones:
(a) 8 in per frame position, 16 out per data symbol; (b) strip 8 in per position + 16 out
per symbol, equalise 32 per symbol; (c) 32 per symbol.

  python tools/pilot_csi_measure.py [--mods 16QAM 256QAM --batch 1048576 --rounds 5] [--out f.json]"""
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


def measure(mod, a, dev):
    codec = M.DVBRCS2_Turbo(a.n, a.rate, interleaver="valid-perm", device=0)
    B = a.batch
    lay = D.PilotLayout(a.plen, a.dlen)
    _, frames, n0, _ = make_symbols(codec, B, mod, a.ebn0, 99, dev, want_info=False, fading={"K": 0.0, "coh": 1 << 20},
                                    pilots=lay, cfo=a.cfo)
    T = frames.shape[1]
    S = -(-codec.handle.enc_len // D.MODULATIONS[mod]["bps"])
    z, nvs = torch.empty((B, S), dtype=torch.complex64, device=dev), torch.empty((B, S), dtype=torch.float64, device=dev)
    y, h = torch.empty_like(z), torch.empty_like(z)
    z2, nvs2 = torch.empty_like(z), torch.empty_like(nvs)
    st = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def unfused():
        D.strip_pilots_device(frames, lay, out=y, h_out=h)
        D.equalize_device(y, h, n0, coh=1, out=z2, nv_out=nvs2)

    variants = [("fused", lambda: D.estimate_csi_device(frames, lay, n0, out=z, nv_out=nvs)),
                ("fused, estimated noise", lambda: D.estimate_csi_device(frames, lay, None, out=z, nv_out=nvs)),
                ("unfused", unfused),
                ("strip alone", lambda: D.strip_pilots_device(frames, lay, out=y, h_out=h)),
                ("equaliser alone", lambda: D.equalize_device(y, h, n0, coh=1, out=z2, nv_out=nvs2))]
    times = {k: [] for k, _ in variants}
    for r in range(2 * a.rounds + 1):                  # round 0 untimed; odd rounds forward, even rounds reversed
        for k, fn in (variants if r % 2 else variants[::-1]):
            t = timed(fn)
            if r:
                times[k].append(t)
    D.estimate_csi_device(frames, lay, n0, out=z, nv_out=nvs)
    unfused()
    torch.cuda.synchronize()
    same = bool(torch.equal(z.view(torch.int64), z2.view(torch.int64)) and
                torch.equal(nvs.view(torch.int64), nvs2.view(torch.int64)))
    assert same, f"{mod}: fused and unfused outputs differ"
    ms = {k: stats(t) for k, t in times.items()}
    n_sym, n_pos = B * S, B * T
    by = {"fused": 8.0 * n_pos + 16.0 * n_sym, "fused, estimated noise": 8.0 * n_pos + 16.0 * n_sym,
          "unfused": 8.0 * n_pos + 16.0 * n_sym + 32.0 * n_sym, "strip alone": 8.0 * n_pos + 16.0 * n_sym,
          "equaliser alone": 32.0 * n_sym}
    rec = {"mod": mod, "n_couples": a.n, "rate": a.rate, "codewords": B, "data_symbols": S, "frame_len": T,
           "plen": a.plen, "dlen": a.dlen, "cfo": a.cfo, "ebn0_db": a.ebn0, "rounds_each_order": a.rounds,
           "fused_equals_unfused": same, "ms": ms, "bytes": by,
           "tb_per_s": {k: by[k] / (ms[k]["median"] * 1e-3) / 1e12 for k in ms},
           "fused_over_unfused": ms["fused"]["median"] / ms["unfused"]["median"],
           "fused_over_equaliser": ms["fused"]["median"] / ms["equaliser alone"]["median"]}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mods", nargs="+", default=["16QAM", "256QAM"])
    ap.add_argument("--n", type=int, default=752)
    ap.add_argument("--rate", default="1/3")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ebn0", type=float, default=2.0)
    ap.add_argument("--plen", type=int, default=4)
    ap.add_argument("--dlen", type=int, default=47)
    ap.add_argument("--cfo", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    recs = []
    for m in a.mods:
        recs.append(measure(m, a, dev))
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
