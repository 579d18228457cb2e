"""Coded-BER Monte-Carlo sweep on MI355X (BASELINE.json configs[3]/[4]):
Eb/N0 points x codewords, sharded over GPUs with torchrun, resumable.

  python -m modulations_amd.ber --mod 256QAM --n 752 --rate 1/3 --ebn0=-2:10:1 \
      --codewords 10000000 --out ber_256qam.json
  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m modulations_amd.ber ...

Each rank owns a contiguous range of global codeword indices per point
(sharding.shard_range) and generates it on its own device with the
counter-based generator (seed per point, counter = global codeword index: the
data, and so the counters, are the same for any world size or batch size),
runs the fused demap + decode, and counts bit / frame errors on the device;
only those int64 counters are all-reduced.  Finished points are written to
--out after every point, and a rerun skips them (checkpoint / resume, SURVEY
§5).  The file records the sweep's configuration and the generator version;
a rerun into it with any other configuration (modulation, block size, rate,
algorithm, iterations, interleaver, codewords per point, base seed, early
stop and its decoder, demapper, channel, receive branches) or generator is refused instead of mixing two data streams, and each point's
generator key is derived from its Eb/N0 value (not its index in --ebn0), so a
resumed sweep over a different grid regenerates exactly the same data.

--channel rayleigh | rician (with --rician-k, --coherence) sweeps a flat-fading
channel with known gains: the generator multiplies each symbol by
its gain (E|h|^2 = 1, one gain per --coherence symbols of a codeword), and the
pipeline equalises and demaps with the per-symbol noise variance N0 / |h|^2.  The
bits and the noise are those of the AWGN sweep with the same seed.

--csi pilots (fading channels) frames each burst with pilot blocks
(--pilot-len symbols every --pilot-spacing data symbols, --cfo cycles per symbol of residual
carrier rotation at most) and lets the pipeline estimate the gains from them, with the
noise variance known (--csi-noise known) or estimated from the pilots as well (pilots).
The pilots' energy is not charged to Eb/N0.

--rx-branches R (fading channels) receives every burst on R independently
faded, independently noisy branches and combines them (maximal ratio) in front of the
demapper, with --csi known or pilots.  Eb/N0 is per branch: the array gain (10 log10 R dB
of collected energy) is not charged, so the curves show it together with the diversity gain.

--tx-antennas 2 (fading channels, --csi known) sends every codeword from two
antennas with the Alamouti space-time block code and combines the R = --rx-branches branches'
pairs of slots in front of the demapper; with --llr, --demap and --early-stop as without it.
--coherence counts slots and must be even.  Eb/N0 is per receive branch at fixed total transmit
power: the two antennas share it.  Recorded in the sweep configuration only when 2.

--tx-antennas 2 --tx-mode sm multiplexes instead: the two antennas send two
different symbols in every slot and the R = --rx-branches branches are detected jointly (max-log
over the M^2 hypotheses of a slot; up to 64QAM); with --llr and --early-stop as without it,
--coherence counts slots and may be odd.  Eb/N0 is per receive branch at fixed total transmit
power, as for the block code; the doubled rate is not charged.  Recorded in the sweep
configuration only when sm.

--harq chase | ir with --max-tx T sends a codeword again while its decode is
wrong, up to T transmissions, and soft-combines them (workload.HarqPipeline): chase repeats
the --rate pattern, ir cycles through its redundancy versions into a rate-1/3 decoder.  The
ACK is genie-aided (the error count against the known info bits).  awgn or a fading channel
with known gains, one branch; every transmission has fresh noise and gains.  Eb/N0 is per
transmission: the retransmissions' energy is not charged, mean_tx says how many there were.
Each point records the residual BER / FER after T, tx_hist and mean_tx.

--crc crc16 | crc32 puts a check field into the last r info bits of every
codeword (crc.attach_device) and verifies the decoded bits on the device (crc.check_device).  A
point then reports what a link sees: the payload BER, the FER (frames with a wrong bit, payload
or check field), crc_fail (frames the check rejects) and undetected (frames that pass it with a
payload bit error); fer = (crc_fail + undetected) / codewords.  With --harq, --ack crc lets the
check drive the retransmissions (a row is sent again while it fails) in place of the genie
(--ack genie, the default, which then compares with the info bits that carry the check field);
the two can differ only on undetected rows.  The rate loss of the check field is not charged to
Eb/N0, as for pilots.

--llr int8 | f16 puts a soft-bit link between demapper and decoder: the flat
demapper's LLRs are narrowed to int8 (demap.quantize_llr_device with --llr-step, default
float32(30 / 127)) or float16 and widened again by the de-puncture kernel.  --llr f32 (default)
is the plane demapper as before and leaves the sweep configuration as it was.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np


GENERATOR = "philox4x32-10/global-codeword-index/v2"   # workload.make_symbols' stream; bump on any change


def ebn0_seed(base_seed, ebn0_db):
    """Generator key of the point at `ebn0_db`: the base seed and the Eb/N0
    value in milli-dB, so the key does not depend on the point's position in
    the sweep grid (64-bit, as the device generator takes it)."""
    return (int(base_seed) * 1_000_003 + int(round(float(ebn0_db) * 1000)) * 7919) & 0xFFFFFFFFFFFFFFFF


def sweep_config(a, inv_perm=None):
    """What a results file is keyed on (argparse namespace -> dict), including the
    digest of the inverse interleaver actually used (sharding.interleaver_digest:
    the reference's default differs between numpy builds)."""
    from .sharding import interleaver_digest
    cfg = {"generator": GENERATOR, "mod": a.mod, "n_couples": int(a.n), "rate": a.rate, "algo": a.algo,
           "iterations": int(a.iterations), "interleaver": a.interleaver, "codewords": int(a.codewords),
           "seed": int(a.seed)}
    if getattr(a, "early_stop", False):   # (absent without the flag: files of earlier sweeps keep resuming)
        cfg["early_stop"] = True
        if getattr(a, "es_decoder", "frame") != "frame":   # (absent at the default, likewise)
            cfg["es_decoder"] = a.es_decoder
    if getattr(a, "demap", "max-log") != "max-log":   # (absent at the default, likewise)
        cfg["demap"] = a.demap
    fading = channel_fading(a)
    if fading is not None:   # (absent for awgn, likewise)
        cfg["channel"] = a.channel
        cfg["rician_k"] = fading["K"]
        cfg["coherence"] = fading["coh"]
        if getattr(a, "csi", "known") == "pilots":   # (absent at the default, likewise)
            cfg.update(csi="pilots", pilot_len=int(a.pilot_len), pilot_spacing=int(a.pilot_spacing),
                       cfo=float(a.cfo), csi_noise=a.csi_noise)
        if "branches" in fading:   # (absent for one branch, likewise)
            cfg["rx_branches"] = fading["branches"]
        if "tx_antennas" in fading:   # (absent for one antenna, likewise)
            cfg["tx_antennas"] = fading["tx_antennas"]
        if sm_mode(a):   # (absent for the block code: files of earlier sweeps keep resuming)
            cfg.update(tx_antennas=2, tx_mode="sm")
    if getattr(a, "harq", None):   # (absent without the flag, likewise)
        cfg.update(harq=a.harq, max_tx=int(a.max_tx))
    if getattr(a, "crc", None):   # (absent without the flag, likewise)
        cfg["crc"] = a.crc
    if getattr(a, "ack", None):   # (absent unless given, likewise)
        cfg["ack"] = a.ack
    if getattr(a, "llr", "f32") != "f32":   # (absent at the default, likewise)
        cfg["llr"] = a.llr
        cfg["llr_step"] = llr_step_of(a)
    if inv_perm is not None:
        cfg["inv_perm_digest"] = interleaver_digest(inv_perm)
    return cfg


def llr_step_of(a):
    """The step of the sweep's --llr link as the configuration records it: the float32 value int8
    rows are widened with (--llr-step, default float32(30 / 127)), 1.0 for f16 (it has none)."""
    from ._native import LLRQ_DEFAULT_STEP
    if a.llr != "int8":
        return 1.0
    step = getattr(a, "llr_step", None)
    return float(LLRQ_DEFAULT_STEP if step is None else np.float32(step))


def sm_mode(a):
    """Whether the sweep multiplexes its two transmit antennas (--tx-antennas 2 --tx-mode sm)."""
    return int(getattr(a, "tx_antennas", 1)) == 2 and getattr(a, "tx_mode", "stbc") == "sm"


def channel_fading(a):
    """workload.make_symbols' `fading` for the sweep's --channel (None: awgn).  rayleigh is
    rician with K = 0, whatever --rician-k says.  A multiplexed link (sm_mode) goes without the
    "tx_antennas" key: make_symbols takes it as streams=2."""
    channel = getattr(a, "channel", "awgn")
    if channel == "awgn":
        return None
    fading = {"K": float(a.rician_k) if channel == "rician" else 0.0, "coh": int(a.coherence)}
    if int(getattr(a, "rx_branches", 1)) > 1:   # (one branch is the call without the key: the same data)
        fading["branches"] = int(a.rx_branches)
    if int(getattr(a, "tx_antennas", 1)) == 2 and not sm_mode(a):   # (one antenna is the call without the key, likewise)
        fading["tx_antennas"] = 2
    return fading


def load_resume(path, cfg):
    """Finished points of `path` for the sweep configuration `cfg`:
    {ebn0_db: record}.  A missing file is an empty sweep; a file written for
    another configuration or generator (or in the old unkeyed list format)
    raises ValueError rather than silently merging points of two streams."""
    if not path or not os.path.exists(path):
        return {}
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or "config" not in doc:
        raise ValueError(f"{path}: results without a sweep configuration (old format); use another --out")
    if doc["config"] != cfg:
        diff = {k: (doc["config"].get(k), cfg.get(k)) for k in set(doc["config"]) | set(cfg)
                if doc["config"].get(k) != cfg.get(k)}
        raise ValueError(f"{path}: written for another sweep configuration {diff} (file, this run); use another --out")
    return {float(r["ebn0_db"]): r for r in doc["points"]}


def save_results(path, cfg, results):
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump({"config": cfg, "points": sorted(results, key=lambda r: r["ebn0_db"])}, f, indent=1)
    os.replace(tmp, path)


def parse_points(spec):
    if ":" in spec:
        a, b, s = (float(x) for x in spec.split(":"))
        return [round(a + i * s, 6) for i in range(int(round((b - a) / s)) + 1)]
    return [float(x) for x in spec.split(",")]


def frame_check_counts(bits, info, kind, ok=None):
    """int64 [5] on the device: payload bit errors, frames with a wrong bit anywhere (payload or
    check field: what the genie NACKs), frames, frames the check rejects, frames that pass it
    with a payload bit error -- decoded `bits` (int32 [n, 2N]) against the info bits that carry
    the check field (uint8 [n, 2N]); ok: the rows' frame check where it has been taken already.
    An error confined to the check field is a burst of at most r bits, which the check rejects,
    so frames in error = rejected + undetected."""
    import torch
    from . import crc as CRC
    payload = bits.shape[1] - CRC.KINDS[kind]["r"]
    wrong = bits != info
    e = wrong[:, :payload].sum(dim=1)
    ok = CRC.check_device(bits, kind) if ok is None else ok
    return torch.stack([e.sum(), wrong.any(dim=1).sum(), torch.tensor(bits.shape[0], device=bits.device),
                        (ok == 0).sum(), ((ok != 0) & (e > 0)).sum()]).to(torch.int64)


def run_point(pipe, codec, mod, ebn0, start, count, batch, seed, device, times=None, iter_hist=None, fading=None,
              pilots=None, crc=None, sm=False):
    """Bit errors, frame errors and codewords of global codewords
    [start, start + count) at one Eb/N0 point.  The data of codeword g is a
    counter-based stream of (seed, g) (workload.make_symbols), so the counters
    do not depend on the batch size or on how the job is sharded.  times (a list,
    optional): per batch, (demap + decode ms, decode ms) from HIP events on the
    pipeline's stream -- the bench's timed step, without the generator and the
    error counting.  iter_hist (an int64 [iterations + 1] device tensor, optional;
    early-stop pipelines): entry i gains the codewords that ran i iterations.
    fading (make_symbols' dict, optional): the flat-fading channel; the pipeline (built
    with csi=True) equalises with the generator's gains.  pilots (optional, with fading):
    {"layout": demap.PilotLayout, "cfo": cycles per symbol, "noise": "known" | "pilots"}: the
    bursts are framed and the pipeline estimates the gains (and the noise) from the pilots.
    fading["branches"] = R: symbols, gains and frames are [n, R, ...] and the pipeline combines.
    crc (a kind, optional; neither pilots nor branches): the codewords carry a check field and the
    counters are frame_check_counts' five.  sm (with fading; neither pilots nor crc): the link is
    spatially multiplexed (make_symbols' streams=2) and the pipeline, built with sm=True, detects jointly."""
    import torch
    from . import sharding as S
    from .workload import count_errors, make_symbols
    cnt = torch.zeros(5 if crc else 3, dtype=torch.int64, device=device)
    ev = []
    for off, n in S.batches(count, batch):
        csi, info = {}, None
        if crc:
            info, syms, n0, *gains = make_symbols(codec, n, mod, ebn0, seed, device, cw0=start + off, fading=fading,
                                                  crc=crc)
            if fading is not None:
                csi = {"csi": gains[0], "coh": fading["coh"]}
        elif fading is None:
            _, syms, n0 = make_symbols(codec, n, mod, ebn0, seed, device, cw0=start + off, want_info=False)
        elif sm:
            _, syms, n0, gains = make_symbols(codec, n, mod, ebn0, seed, device, cw0=start + off, want_info=False,
                                              fading=fading, streams=2)
        elif pilots is not None:
            _, syms, n0, _ = make_symbols(codec, n, mod, ebn0, seed, device, cw0=start + off, want_info=False,
                                          fading=fading, pilots=pilots["layout"], cfo=pilots["cfo"])
        else:
            _, syms, n0, gains = make_symbols(codec, n, mod, ebn0, seed, device, cw0=start + off, want_info=False,
                                              fading=fading)
            csi = {"csi": gains, "coh": fading["coh"]}
        e3 = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e3[0].record()
        if sm:
            bits = pipe.run_sm(syms, n0, gains, coh=fading["coh"], events=e3[1:])[:n]
        elif pilots is not None:
            bits = pipe.run_frames(syms, pilots["layout"], n0 if pilots["noise"] == "known" else None,
                                   events=e3[1:])[:n]
        else:
            bits = pipe.run(syms, n0, events=e3[1:], **csi)[:n]
        ev.append(e3)
        if iter_hist is not None:
            iter_hist += torch.bincount(pipe.n_iter[:n], minlength=iter_hist.numel())[:iter_hist.numel()]
        if crc:
            cnt += frame_check_counts(bits, info, crc)
            continue
        e = count_errors(codec, bits, seed, cw0=start + off)
        cnt += torch.stack([e.sum(dtype=torch.int64), (e > 0).sum(), torch.tensor(n, device=device)]).to(torch.int64)
    if times is not None:
        torch.cuda.synchronize()
        times += [(a.elapsed_time(c), b.elapsed_time(c)) for a, b, c in ev]
    return cnt


def run_point_harq(pipe, mod, ebn0, start, count, batch, seed, device, tx_hist, fading=None, crc=None, ack="genie"):
    """run_point through a workload.HarqPipeline: global codewords [start, start + count) are sent up
    to pipe.max_tx times, a row again while its decode has bit errors (genie-aided ACK), each
    transmission with its codec (pipe.codec(t)), fresh noise and fresh gains.  Returns the residual
    counters; tx_hist (int64 [max_tx + 1] device tensor) gains at entry i the codewords that used i
    transmissions (the ones still wrong after the last count there).
    crc (a kind; a pipeline built with crc=): the codewords carry a check field, the genie compares
    the decoded rows against the attached info bits, and the counters are frame_check_counts' five.
    ack="crc" then sends a row again while the pipeline's own frame check rejects it (receive()
    without `active`: no decision comes from the host)."""
    import torch
    from . import demap as D
    from . import sharding as S
    from .workload import count_errors, make_symbols
    cnt = torch.zeros(5 if crc else 3, dtype=torch.int64, device=device)
    for off, n in S.batches(count, batch):
        active, used, e, info = None, torch.zeros(n, dtype=torch.int64, device=device), None, None
        for t in range(pipe.max_tx):
            out = make_symbols(pipe.codec(t), n, mod, ebn0, seed, device, cw0=start + off,
                               want_info=bool(crc) and t == 0, fading=fading, tx=t, crc=crc)
            info = out[0] if t == 0 else info
            given = None if ack == "crc" else active
            if fading is None:
                bits = pipe.receive(t, out[1], out[2], active=given)
            else:
                z, nvs = D.equalize_device(out[1], out[3], out[2], coh=fading["coh"])
                bits = pipe.receive(t, z, nvs, active=given)
            used += 1 if active is None else active
            if ack == "crc":
                active = pipe.ack[:n] == 0
            elif crc:   # the genie: any wrong bit of the row, check field included
                active = (bits != info).any(dim=1)
            else:
                e = count_errors(pipe.mother, bits, seed, cw0=start + off)
                active = e != 0
            if not bool(active.any()):   # (the tool's only host round trip: nothing left to send)
                break
        tx_hist += torch.bincount(used, minlength=tx_hist.numel())[:tx_hist.numel()]
        if crc:
            cnt += frame_check_counts(bits, info, crc, ok=pipe.ack[:n])
            continue
        cnt += torch.stack([e.sum(dtype=torch.int64), (e > 0).sum(), torch.tensor(n, device=device)]).to(torch.int64)
    return cnt


def _payload_bits(codec, kind):
    from . import crc as CRC
    return CRC.payload_bits(codec, kind)


def arg_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mod", default="256QAM")
    ap.add_argument("--n", "--couples", dest="n", type=int, default=752)
    ap.add_argument("--rate", default="1/3")
    ap.add_argument("--algo", default="max-log")
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--ebn0", default="-2:10:1")
    ap.add_argument("--codewords", type=int, default=1_000_000, help="per Eb/N0 point, whole job")
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--interleaver", default="reference")
    ap.add_argument("--early-stop", action="store_true",
                    help="stop each codeword once its hard decisions repeat (--iterations is the cap); "
                         "records mean_iters and iter_hist per point")
    ap.add_argument("--es-decoder", choices=["frame", "tile", "refill"], default="frame",
                    help="with --early-stop: the frame decoder (default), the throughput tile decoder, or "
                         "the tile decoder that refills finished lanes")
    ap.add_argument("--demap", choices=["max-log", "log-map"], default="max-log",
                    help="the soft demapper in front of the decoder: the reference's max-log, or the exact "
                         "log-sum it approximates")
    ap.add_argument("--channel", choices=["awgn", "rayleigh", "rician"], default="awgn",
                    help="awgn, or flat fading with known gains (E|h|^2 = 1): equalised, then demapped with "
                         "the per-symbol noise variance N0 / |h|^2")
    ap.add_argument("--rician-k", type=float, default=4.0, help="--channel rician: the K factor (linear, >= 0)")
    ap.add_argument("--coherence", type=int, default=1,
                    help="fading channels: symbols per gain (1: fast fading; >= the symbols of a codeword: "
                         "one gain per burst)")
    ap.add_argument("--csi", choices=["known", "pilots"], default="known",
                    help="fading channels: equalise with the generator's gains, or frame the bursts with pilot "
                         "blocks and estimate the gains from them")
    ap.add_argument("--pilot-len", type=int, default=4, help="--csi pilots: symbols per pilot block")
    ap.add_argument("--pilot-spacing", type=int, default=47, help="--csi pilots: data symbols between pilot blocks")
    ap.add_argument("--cfo", type=float, default=0.0,
                    help="--csi pilots: residual carrier rotation, uniform in (-cfo, cfo) cycles per symbol per burst")
    ap.add_argument("--csi-noise", choices=["known", "pilots"], default="known",
                    help="--csi pilots: the noise variance is N0, or each burst's estimate from its pilots")
    ap.add_argument("--rx-branches", type=int, default=1,
                    help="fading channels: receive branches per burst (1 .. 8), independently faded and noisy, "
                         "maximal-ratio combined in front of the demapper; Eb/N0 is per branch (the array gain "
                         "is not charged)")
    ap.add_argument("--tx-antennas", type=int, default=1,
                    help="fading channels, --csi known: transmit antennas (1 or 2).  2 sends every codeword with the "
                         "Alamouti space-time block code (DESIGN.md §18); --coherence then counts slots and must be "
                         "even.  Eb/N0 is per receive branch at fixed total transmit power: the antennas share it")
    ap.add_argument("--tx-mode", choices=["stbc", "sm"], default="stbc",
                    help="--tx-antennas 2: stbc (the default) sends the Alamouti block code, one symbol per slot; sm "
                         "multiplexes, two symbols per slot, detected jointly over the receive branches (max-log, up "
                         "to 64QAM; DESIGN.md §19); --coherence then counts slots and may be odd.  Eb/N0 stays per "
                         "receive branch at fixed total transmit power: the doubled rate is not charged")
    ap.add_argument("--harq", choices=["chase", "ir"], default=None,
                    help="hybrid ARQ with a genie-aided ACK: resend a codeword while its decode is wrong and "
                         "soft-combine; chase repeats the pattern, ir cycles its redundancy versions into a "
                         "rate-1/3 decoder (known CSI, one branch)")
    ap.add_argument("--max-tx", type=int, default=4, help="--harq: transmissions per codeword at most")
    ap.add_argument("--crc", choices=["crc16", "crc32"], default=None,
                    help="attach this check field to the info bits of every codeword and verify the decoded bits on "
                         "the device: a point reports the payload BER, FER, crc_fail and undetected (frames that "
                         "pass the check with a payload bit error).  The check field's rate loss is not charged to "
                         "Eb/N0, as for pilots (--csi known, one receive branch)")
    ap.add_argument("--ack", choices=["genie", "crc"], default=None,
                    help="--harq: what asks for a retransmission -- the comparison with the known info bits "
                         "(genie, the default), or the frame check of --crc on the decoded bits (crc)")
    ap.add_argument("--llr", choices=["f32", "int8", "f16"], default="f32",
                    help="the soft-bit link between demapper and decoder (DESIGN.md §17): f32 (the plane demapper, "
                         "no link), or the flat demapper's LLRs narrowed to int8 (--llr-step) or float16 and widened "
                         "by the de-puncture kernel")
    ap.add_argument("--llr-step", type=float, default=None,
                    help="--llr int8: the LLR value of one quantiser step (default 30 / 127 as float32)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL) on the node; gloo to rehearse")
    ap.add_argument("--all-on-device0", action="store_true", help="every rank on GPU 0 (rehearsal on a 1-GPU box)")
    ap.add_argument("--dist-timeout", type=float, default=300.0, help="torch.distributed timeout (s)")
    return ap


def main(argv=None):
    import torch
    import torch.distributed as dist
    from . import dvb_rcs2_turbo as M
    from . import sharding as S
    from .workload import DevicePipeline, HarqPipeline

    ap = arg_parser()
    a = ap.parse_args(argv)
    if a.harq and (a.csi == "pilots" or a.rx_branches > 1 or not 1 <= a.max_tx <= 65536):
        ap.error("--harq takes --csi known, one receive branch and 1 <= --max-tx <= 65536")
    if a.ack and not a.harq:
        ap.error("--ack needs --harq")
    if a.ack == "crc" and not a.crc:
        ap.error("--ack crc needs --crc")
    if a.crc and (a.csi == "pilots" or a.rx_branches > 1):
        ap.error("--crc takes --csi known and one receive branch")
    if a.coherence < 1 or not (0.0 <= a.rician_k < float("inf")):
        ap.error("--coherence must be >= 1 and --rician-k a finite value >= 0")
    if not 1 <= a.rx_branches <= 8:
        ap.error("--rx-branches must be 1 .. 8")
    if a.rx_branches > 1 and a.channel == "awgn":
        ap.error("--rx-branches needs --channel rayleigh or rician")
    if a.tx_antennas not in (1, 2):
        ap.error("--tx-antennas must be 1 or 2")
    if a.tx_antennas == 2:
        if a.channel == "awgn" or a.csi != "known":
            ap.error("--tx-antennas 2 needs --channel rayleigh or rician and --csi known")
        if a.harq or a.crc:
            ap.error("--tx-antennas 2 takes neither --harq nor --crc")
        if a.tx_mode == "sm":
            if a.demap != "max-log":
                ap.error("--tx-mode sm detects jointly with max-log only: it takes no --demap log-map")
            if a.mod == "256QAM":
                ap.error("--tx-mode sm detects up to 64QAM jointly")
        elif a.coherence < 2 or a.coherence % 2:
            ap.error("--tx-antennas 2 needs an even --coherence (a pair of slots shares its gains)")
    if a.tx_mode == "sm" and a.tx_antennas != 2:
        ap.error("--tx-mode sm needs --tx-antennas 2")
    if a.llr_step is not None and (a.llr != "int8" or not 0.0 < a.llr_step < float("inf")):
        ap.error("--llr-step goes with --llr int8 and must be a finite value > 0")
    fading = channel_fading(a)
    pilots = None
    if a.csi == "pilots":
        from .demap import PilotLayout
        if fading is None:
            ap.error("--csi pilots needs a fading --channel")
        if a.pilot_len < 1 or a.pilot_spacing < 1 or not (0.0 <= a.cfo < float("inf")):
            ap.error("--pilot-len and --pilot-spacing must be >= 1 and --cfo a finite value >= 0")
        if a.csi_noise == "pilots" and a.pilot_len < 2:
            ap.error("--csi-noise pilots needs --pilot-len >= 2")
        pilots = {"layout": PilotLayout(a.pilot_len, a.pilot_spacing), "cfo": a.cfo, "noise": a.csi_noise}

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.all_on_device0 and world > 1 and a.dist_backend == "nccl":
        ap.error("--all-on-device0 puts several ranks on one GPU, which RCCL cannot do: add --dist-backend gloo")
    # the codec touches no GPU until its first call: its inv_perm keys the sweep
    try:
        host_codec = M.DVBRCS2_Turbo(a.n, a.rate, a.iterations, algo=a.algo, interleaver=a.interleaver,
                                     early_stop=a.early_stop, es_decoder=a.es_decoder)
    except ValueError as e:
        ap.error(str(e))
    cfg = sweep_config(a, host_codec.inv_perm)
    try:
        done = load_resume(a.out, cfg)
    except ValueError as e:
        ap.error(str(e))
    dev_idx = 0 if a.all_on_device0 else local
    torch.cuda.set_device(dev_idx)
    if world > 1:
        import datetime
        to = datetime.timedelta(seconds=a.dist_timeout)
        if a.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_idx), timeout=to)
        else:
            dist.init_process_group(a.dist_backend, timeout=to)
    device = torch.device("cuda", dev_idx)
    codec = M.DVBRCS2_Turbo(a.n, a.rate, a.iterations, algo=a.algo, interleaver=a.interleaver,
                            device=device.index, early_stop=a.early_stop, es_decoder=a.es_decoder)
    if world > 1:   # every rank must decode with the same de-interleaver
        S.check_same_interleaver(codec.inv_perm, dist, device if a.dist_backend == "nccl" else "cpu")
    results = list(done.values())
    if a.harq:
        kw = dict(algo=a.algo, interleaver=a.interleaver, device=device.index)
        versions = range(codec.punct["period"]) if a.harq == "ir" else (0,)
        codecs = [codec if r == 0 else M.DVBRCS2_Turbo(a.n, a.rate, a.iterations, rv=r, **kw) for r in versions]
        mother = codec if a.harq == "chase" else M.DVBRCS2_Turbo(a.n, "1/3", a.iterations, early_stop=a.early_stop,
                                                                 es_decoder=a.es_decoder, **kw)
        pipe = HarqPipeline(codecs, mother, a.mod, a.batch, device, demap=a.demap, max_tx=a.max_tx, crc=a.crc,
                            llr=a.llr, llr_step=a.llr_step)
        run_point_harq(pipe, a.mod, 2.0, 0, min(a.batch, 65536), a.batch, a.seed, device,
                       torch.zeros(a.max_tx + 1, dtype=torch.int64, device=device), fading=fading, crc=a.crc,
                       ack=a.ack or "genie")
    else:
        pipe = DevicePipeline(codec, a.mod, a.batch, device, demap=a.demap, csi=fading is not None and not sm_mode(a),
                              llr=a.llr, llr_step=a.llr_step, sm=sm_mode(a))
        # one untimed batch first: code-object loading and first-launch costs stay out of
        # the first point's figures
        run_point(pipe, codec, a.mod, 2.0, 0, min(a.batch, 65536), a.batch, a.seed, device, fading=fading,
                  pilots=pilots, crc=a.crc, sm=sm_mode(a))
    for e in parse_points(a.ebn0):
        if e in done:
            continue
        start, count = S.shard_range(a.codewords, world, rank)
        t0 = time.time()
        times = []
        hist = torch.zeros(a.iterations + 1, dtype=torch.int64, device=device) if a.early_stop else None
        if a.harq:   # (no iteration histogram: a row is decoded once per transmission)
            hist = torch.zeros(a.max_tx + 1, dtype=torch.int64, device=device)
            cnt = run_point_harq(pipe, a.mod, e, start, count, a.batch, ebn0_seed(a.seed, e), device, hist,
                                 fading=fading, crc=a.crc, ack=a.ack or "genie")
        else:
            cnt = run_point(pipe, codec, a.mod, e, start, count, a.batch, ebn0_seed(a.seed, e), device, times, hist,
                            fading=fading, pilots=pilots, crc=a.crc, sm=sm_mode(a))
        nc = 5 if a.crc else 3   # the error counters in front of the histogram
        if hist is not None:
            cnt = torch.cat([cnt, hist])   # one reduction for the error counters and the histogram
        if world > 1 and a.dist_backend != "nccl":
            cnt = cnt.cpu()
        S.reduce_counters(cnt, dist if world > 1 else None)
        torch.cuda.synchronize()
        be, fe, ncw = (int(x) for x in cnt[:3].tolist())
        info_bits = _payload_bits(codec, a.crc) if a.crc else codec.k_info   # the bits `ber` is over
        dt = time.time() - t0
        rec = {"ebn0_db": e, "mod": a.mod, "n_couples": a.n, "rate": a.rate, "algo": a.algo,
               "interleaver": a.interleaver, "codewords": ncw,
               "bit_errors": be, "frame_errors": fe, "ber": be / (ncw * info_bits), "fer": fe / ncw,
               "seconds": dt, "codewords_per_s": ncw / dt, "gpus": world,
               # this rank's demap + decode (the bench's step) and decode alone, HIP events
               "step_ms": sum(t[0] for t in times), "decode_ms": sum(t[1] for t in times),
               "step_codewords_per_s": count / max(1e-9, sum(t[0] for t in times) * 1e-3),
               "decode_codewords_per_s": count / max(1e-9, sum(t[1] for t in times) * 1e-3)}
        if a.demap != "max-log":
            rec["demap"] = a.demap
        if a.llr != "f32":
            rec.update(llr=a.llr, llr_step=llr_step_of(a))
        if fading is not None:
            rec.update(channel=a.channel, rician_k=fading["K"], coherence=fading["coh"])
            if "branches" in fading:
                rec["rx_branches"] = fading["branches"]
            if "tx_antennas" in fading:
                rec["tx_antennas"] = fading["tx_antennas"]
            if sm_mode(a):
                rec.update(tx_antennas=2, tx_mode="sm")
        if pilots is not None:
            rec.update(csi="pilots", pilot_len=a.pilot_len, pilot_spacing=a.pilot_spacing, cfo=a.cfo,
                       csi_noise=a.csi_noise)
        if a.harq:
            h = [int(x) for x in cnt[nc:].tolist()]
            for k in ("step_ms", "decode_ms", "step_codewords_per_s", "decode_codewords_per_s"):
                del rec[k]   # (the bench step's figures: not taken here)
            # ber / fer are the residual ones after max_tx; tx_hist[i]: codewords that used i transmissions
            rec.update(harq=a.harq, max_tx=a.max_tx, tx_hist=h,
                       mean_tx=sum(i * c for i, c in enumerate(h)) / max(1, ncw))
            if a.early_stop:
                rec["early_stop"] = True
        elif a.early_stop:
            h = [int(x) for x in cnt[nc:].tolist()]
            rec["early_stop"] = True
            if a.es_decoder != "frame":
                rec["es_decoder"] = a.es_decoder
            rec["iter_hist"] = h   # iter_hist[i]: codewords that ran i iterations
            rec["mean_iters"] = sum(i * c for i, c in enumerate(h)) / max(1, ncw)
        if a.crc:   # ber is the payload's; fer: frames with a wrong bit, check field included
            rec.update(crc=a.crc, payload_bits=info_bits, crc_fail=int(cnt[3]), undetected=int(cnt[4]))
            if a.harq:
                rec["ack"] = a.ack or "genie"
        results.append(rec)
        if rank == 0:
            print(json.dumps(rec), flush=True)
            if a.out:
                save_results(a.out, cfg, results)
    if world > 1:
        dist.destroy_process_group()
    return results


if __name__ == "__main__":
    main()
