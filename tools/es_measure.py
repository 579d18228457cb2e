#!/usr/bin/env python3
"""Early-stop measurements, one JSON document on stdout.

  python tools/es_measure.py latency    [--parent lib/libtdec_parent.so]
  python tools/es_measure.py throughput [--batch 65536] [--parent lib/libtdec_parent.so] [--reverse]

latency: one host-pointer decode per call (what DVBRCS2_Turbo.decode() costs below
its numpy conversions: the C call tdec_decode_batch / tdec_decode_batch_es with B = 1)
at N = 48 / 212 / 752 r = 1/3, valid-perm, BPSK LLRs at 2 / 4 / 8 dB, 20 frames per
point, the variants interleaved call by call in one process: this build's plain
decode, this build's early-stop decode and, with --parent, the parent commit's plain
decode (and its early-stop decode, where it has one) from its own library (a second
code object in the same process, as tools/ab.py loads it).  Median ms per call and
the mean n_iter.

throughput: the configs[2] shape (16QAM, N = 752 r = 1/3, valid-perm) at 2, 4 and 6 dB,
device-resident planes: the tile decoder at 8 fixed iterations (tdec_decode_planes_dev;
with --parent also the parent commit's, from its own library), the frame kernel with
early stop (tdec_decode_planes_es_dev), the tile decoder with early stop
(tdec_decode_planes_es_tile_dev) and the tile decoder that refills
finished lanes (tdec_decode_planes_es_refill_dev, §8.3), interleaved round by round, HIP
events: median, min and max ms of --reps rounds, the mean n_iter, the mean over tiles of
the tile's largest n_iter (the iterations the tile decoder runs) and the refill decoder's
trips per wave (tdec_es_refill_stats of its last launch)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from modulations_amd import _native, tables as T  # noqa: E402
from modulations_amd import dvb_rcs2_turbo as M  # noqa: E402


def open_lib(path):
    L = C.CDLL(os.path.abspath(path))
    _native._declare(L)
    return L


def make_handle(L, codec, iters=8):
    tabs = T.packed_tables(codec.next_state, codec.out_W, codec.out_Y, codec.prev_state, codec.prev_input)
    pm = np.ascontiguousarray(T.puncture_matrix(codec.punct))
    h = C.c_void_p()
    rc = L.tdec_create(0, codec.N, codec.punct["period"], pm.ctypes.data, iters, codec.algo, codec.perm.ctypes.data,
                       codec.inv_perm.ctypes.data, tabs.ctypes.data, C.byref(h))
    assert rc == 0, L.tdec_last_error()
    return h


def latency(a):
    import early_stop_ref as R
    cur = _native.lib()
    par = open_lib(a.parent) if a.parent else None
    out = {"what": "host-pointer decode of one frame per call, median ms of the C call", "frames": 20, "reps": a.reps,
           "points": []}
    for n in (48, 212, 752):
        codec = M.DVBRCS2_Turbo(n, "1/3", interleaver="valid-perm")
        hc = make_handle(cur, codec)
        hp = make_handle(par, codec) if par else None
        for ebn0 in (2.0, 4.0, 8.0):
            _, llr = R.bpsk_llrs(codec, np.random.default_rng(n), 20, ebn0)
            bits = np.zeros(codec.k_info, np.int32)
            nit = np.zeros(1, np.int32)
            variants = {"plain": lambda f: cur.tdec_decode_batch(hc, 1, f.ctypes.data, f.size, bits.ctypes.data, None),
                        "early_stop": lambda f: cur.tdec_decode_batch_es(hc, 1, f.ctypes.data, f.size, bits.ctypes.data,
                                                                         None, nit.ctypes.data)}
            if par:
                variants["parent_plain"] = lambda f: par.tdec_decode_batch(hp, 1, f.ctypes.data, f.size,
                                                                           bits.ctypes.data, None)
                if hasattr(par, "tdec_decode_batch_es"):
                    variants["parent_early_stop"] = lambda f: par.tdec_decode_batch_es(hp, 1, f.ctypes.data, f.size,
                                                                                       bits.ctypes.data, None,
                                                                                       nit.ctypes.data)
            order = list(variants)[::-1] if a.reverse else list(variants)
            ts = {k: [] for k in variants}
            its = []
            for rep in range(a.reps + 1):   # the first pass warms up
                for f in llr:
                    for k in order:
                        t0 = time.perf_counter()
                        rc = variants[k](f)
                        dt = time.perf_counter() - t0
                        assert rc == 0
                        if rep:
                            ts[k].append(dt)
                            if k == "early_stop":
                                its.append(int(nit[0]))
            rec = {"N": n, "ebn0_db": ebn0, "order": order, "mean_n_iter": float(np.mean(its))}
            rec.update({k + "_ms": round(float(np.median(v)) * 1e3, 4) for k, v in ts.items()})
            ref = rec.get("parent_plain_ms", rec["plain_ms"])
            rec["early_stop_over_" + ("parent" if par else "plain")] = round(rec["early_stop_ms"] / ref, 3)
            if par:
                rec["plain_over_parent"] = round(rec["plain_ms"] / rec["parent_plain_ms"], 3)
            if "parent_early_stop_ms" in rec:
                rec["early_stop_over_parent_early_stop"] = round(rec["early_stop_ms"] / rec["parent_early_stop_ms"], 3)
            out["points"].append(rec)
        cur.tdec_destroy(hc)
        if par:
            par.tdec_destroy(hp)
    print(json.dumps(out, indent=1))


def throughput(a):
    import torch
    from modulations_amd import demap as D
    from modulations_amd.workload import make_symbols
    dev = torch.device("cuda", 0)
    B = a.batch
    assert B % 64 == 0
    par = open_lib(a.parent) if a.parent else None
    out = {"what": "decode of device-resident planes, HIP events, ms over %d timed rounds, the variants "
                   "interleaved round by round in one process" % a.reps,
           "batch": B, "N": 752, "rate": "1/3", "mod": "16QAM", "interleaver": "valid-perm", "points": []}
    plain = M.DVBRCS2_Turbo(752, "1/3", interleaver="valid-perm")
    frame = M.DVBRCS2_Turbo(752, "1/3", interleaver="valid-perm", early_stop=True)
    tile = M.DVBRCS2_Turbo(752, "1/3", interleaver="valid-perm", early_stop=True, es_decoder="tile")
    cons = D.constellation("16QAM")
    planes = torch.empty(plain.planes_bytes(B) // 4, dtype=torch.float32, device=dev)
    plain.reserve(B)
    tile.reserve(B)
    refill = M.DVBRCS2_Turbo(752, "1/3", interleaver="valid-perm", early_stop=True, es_decoder="refill")
    refill.reserve(B)
    names = ["tile_8_iterations", "frame_early_stop", "tile_early_stop", "refill_early_stop"]
    bits = {k: torch.empty((B, plain.k_info), dtype=torch.int32, device=dev) for k in names}
    nit = {k: torch.zeros(B, dtype=torch.int32, device=dev) for k in names[1:]}
    st = torch.cuda.current_stream()
    fns = {"tile_8_iterations": lambda: plain.decode_planes_device(planes, B, bits["tile_8_iterations"]),
           "frame_early_stop": lambda: frame.decode_planes_device(planes, B, bits["frame_early_stop"],
                                                                  n_iter=nit["frame_early_stop"]),
           "tile_early_stop": lambda: tile.decode_planes_device(planes, B, bits["tile_early_stop"],
                                                                n_iter=nit["tile_early_stop"]),
           "refill_early_stop": lambda: refill.decode_planes_device(planes, B, bits["refill_early_stop"],
                                                                    n_iter=nit["refill_early_stop"])}
    if par:   # the parent commit's fixed tile decoder, from its own library
        hp = make_handle(par, plain)
        assert par.tdec_reserve(hp, B) == 0, par.tdec_last_error()
        bits["parent_tile_8_iterations"] = torch.empty_like(bits["tile_8_iterations"])
        pb = bits["parent_tile_8_iterations"]
        fns["parent_tile_8_iterations"] = lambda: par.tdec_decode_planes_dev(hp, B, planes.data_ptr(), pb.data_ptr(),
                                                                             None, st.cuda_stream)
        names = ["parent_tile_8_iterations"] + names
    if a.skip_frame:
        names.remove("frame_early_stop")
    order = names[::-1] if a.reverse else names
    out["order"] = order
    for ebn0 in (2.0, 4.0, 6.0):
        _, syms, n0 = make_symbols(plain, B, "16QAM", ebn0, 7, dev, want_info=False)
        _, div32, nve = D.demap_mode(np.complex64, cons.dtype, np.float64(n0))
        plain.demap_planes_device(syms, cons, 4, nve, planes, div_f32=div32)
        ms = {k: [] for k in order}
        for rep in range(a.reps + 1):   # the first round warms up
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[k]()
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[k].append(e0.elapsed_time(e1))
        nt = nit["tile_early_stop"]
        rec = {"ebn0_db": ebn0, "mean_n_iter": float(nt.double().mean()),
               # the iterations a tile runs: the work the tile decoder actually does
               "mean_tile_max_n_iter": float(nt.view(-1, 64).max(1).values.double().mean()),
               "rows_where_bits_differ_from_fixed": int((bits["tile_8_iterations"]
                                                         != bits["tile_early_stop"]).any(1).sum()),
               "refill_vs_tile_rows_differing": int(((bits["refill_early_stop"] != bits["tile_early_stop"]).any(1)
                                                     | (nit["refill_early_stop"] != nt)).sum())}
        trips, refills = refill.refill_stats()
        waves = min(B // 64, refill_waves(refill))
        rec["refill_trips"], rec["refill_refills"], rec["refill_waves"] = trips, refills, waves
        rec["refill_trips_per_wave"] = round(trips / waves, 2)
        if not a.skip_frame:
            rec["tile_vs_frame_rows_differing"] = int(((bits["frame_early_stop"] != bits["tile_early_stop"]).any(1)
                                                      | (nit["frame_early_stop"] != nt)).sum())
        for k, v in ms.items():
            rec[k + "_ms"] = round(float(np.median(v)), 3)
            rec[k + "_ms_min_max"] = [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]
            rec[k + "_cw_per_s"] = round(B / (float(np.median(v)) * 1e-3))
        out["points"].append(rec)
    if par:
        par.tdec_destroy(hp)
    print(json.dumps(out, indent=1))


def refill_waves(codec):
    """Persistent waves a large refill launch runs: the resident waves of the decode kernel
    (two per SIMD, eight per CU: its 256 VGPRs and 20 KiB of LDS per wave), or
    TDEC_ES_TILE_WAVES."""
    import torch
    full = 8 * torch.cuda.get_device_properties(codec.device).multi_processor_count
    cap = os.environ.get("TDEC_ES_TILE_WAVES")
    return max(1, min(full, int(cap))) if cap else full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["latency", "throughput"])
    ap.add_argument("--parent", default=None, help="the parent commit's libtdec.so, timed beside this build's")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reverse", action="store_true", help="time the variants in the opposite order")
    ap.add_argument("--skip-frame", action="store_true", help="throughput: leave the frame kernel out")
    ap.add_argument("--batch", type=int, default=65536)
    a = ap.parse_args()
    (latency if a.what == "latency" else throughput)(a)


if __name__ == "__main__":
    main()
