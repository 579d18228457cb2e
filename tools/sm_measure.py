#!/usr/bin/env python3
"""Cost of the joint detector, in one process with HIP events, both orders, on the
generators' slots: sm_detect_dev for each modulation with R = 1, 2, 4 receive branches and common
(scalar) noise, coh = 1 and coh = T, against the cheapest existing 2 x R receive front end on the
same codewords, stbc_combine_dev + tdec_symnv_demap_dev (demap.stbc_combine_device and
demap.compute_llr_device with the per-symbol noise), as the yardstick.

f64 operations per hypothesis (a, b), counted from k_sm_detect's inner loop: per branch two
subtractions (v = u - p), two multiplications and one addition (d_r), and R - 1 additions into D:
6 R - 1, no fused multiply-add (the definition has none).  The minima (bps low-bit v_min per
hypothesis) are counted apart.  The peak the fraction is taken against is the MI355X's public f64
vector figure, 78.6 TFLOP/s, which counts a fused multiply-add as two operations; the
microarchitecture guide this project measures against states no f64 vector figure of its own.

  python tools/sm_measure.py [--mods QPSK 16QAM 64QAM --batch 1048576 --rounds 5] [--out f.json]"""
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

F64_VECTOR_PEAK = 78.6e12                             # public MI355X figure, FMA = 2 operations


def stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}


def measure(mod, coh_burst, a, dev):
    codec = M.DVBRCS2_Turbo(a.n, a.rate, interleaver="valid-perm", device=0)
    bps, order = D.MODULATIONS[mod]["bps"], D.MODULATIONS[mod]["order"]
    S = -(-codec.handle.enc_len // bps)
    T, S2 = (S + 1) // 2, S + (S & 1)
    # a batch whose largest input would exceed max_bytes is cut and its times scaled to --batch codewords:
    # an extrapolation, marked in the record ("scaled")
    st = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    times, run_b = {}, {}
    for R in a.branches:
        c_sm, c_st = (T, S2) if coh_burst else (1, 2)
        # bytes per codeword of everything resident at once: both links' slots and gains, both LLR buffers, z, nv_sym
        per_cw = 8 * R * T + 16 * R * -(-T // c_sm) + 8 * R * S2 + 16 * R * -(-S2 // c_st) + 12 * S * bps + 16 * S
        B = min(a.batch, max(1024, int(a.max_bytes // per_cw)))
        run_b[R] = B
        fading = {"K": 0.0, "branches": R}
        _, ys, n0, hs = make_symbols(codec, B, mod, a.ebn0, 99, dev, want_info=False, fading={**fading, "coh": c_sm}, streams=2)
        _, y2, _, h2 = make_symbols(codec, B, mod, a.ebn0, 99, dev, want_info=False,
                                    fading={**fading, "coh": c_st, "tx_antennas": 2})
        llr32 = torch.full((B, S * bps), float("nan"), dtype=torch.float32, device=dev)   # a sentinel in every LLR
        llr64 = torch.empty((B, S * bps), dtype=torch.float64, device=dev)
        z = torch.empty((B, S), dtype=torch.complex64, device=dev)
        nvs = torch.empty((B, S), dtype=torch.float64, device=dev)

        def yard():
            D.stbc_combine_device(y2, h2, n0, S=S, coh=c_st, out=z, nv_out=nvs)
            D.compute_llr_device(z, mod, nvs, out=llr64, sign=-1)
        variants = [(f"sm R={R}", lambda: D.sm_detect_device(ys, hs, mod, n0, S=S, coh=c_sm, out=llr32, sign=-1)),
                    (f"stbc+demap R={R}", yard)]
        for k, _ in variants:
            times[k] = []
        variants[0][1]()                               # the detector writes no NaN: the whole batch was detected
        if bool(torch.isnan(llr32[-1]).any()) or bool(torch.isnan(llr32).any()):
            raise RuntimeError(f"{mod} R={R}: sm_detect_device left LLRs unwritten")
        for r in range(2 * a.rounds + 1):              # round 0 untimed; odd rounds forward, even rounds reversed
            for k, fn in (variants if r % 2 else variants[::-1]):
                t = timed(fn) * a.batch / B
                if r:
                    times[k].append(t)
        del ys, hs, y2, h2, llr32, llr64, z, nvs
        torch.cuda.empty_cache()
    ms = {k: stats(t) for k, t in times.items()}
    hyp = (S // 2) * order * order + (S & 1) * order   # per codeword
    flop = {f"R={R}": 6 * R - 1 for R in a.branches}
    rec = {"mod": mod, "n_couples": a.n, "rate": a.rate, "codewords": a.batch, "codewords_run": run_b,
           "scaled": {f"R={R}": run_b[R] != a.batch for R in a.branches}, "symbols": S,
           "slots": T, "coh": "T" if coh_burst else 1, "ebn0_db": a.ebn0, "rounds_each_order": a.rounds, "ms": ms,
           "hypotheses_per_codeword": hyp, "f64_ops_per_hypothesis": flop,
           "f64_tflops": {f"R={R}": hyp * a.batch * flop[f"R={R}"] / (ms[f"sm R={R}"]["median"] * 1e-3) / 1e12
                          for R in a.branches},
           "over_stbc_demap": {f"R={R}": ms[f"sm R={R}"]["median"] / ms[f"stbc+demap R={R}"]["median"] for R in a.branches}}
    rec["fraction_of_f64_vector_peak"] = {k: v * 1e12 / F64_VECTOR_PEAK for k, v in rec["f64_tflops"].items()}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mods", nargs="+", default=["QPSK", "16QAM", "64QAM"])
    ap.add_argument("--branches", nargs="+", type=int, default=[1, 2, 4])
    ap.add_argument("--n", type=int, default=752)
    ap.add_argument("--rate", default="1/3")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--max-bytes", type=float, default=200e9,
                    help="device bytes resident at once; a batch that needs more is cut and its times scaled (the "
                         "record's codewords_run and scaled say which rows)")
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
