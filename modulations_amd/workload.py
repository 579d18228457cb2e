"""Device-side synthetic workloads: counter-based (Philox)
info bits -> batched device encoder (encode, dvb_rcs2_turbo.py:404-462) ->
labelled Gray constellation (the reference mappers) -> complex AWGN, and the
per-codeword error counters of a BER point.  Everything stays in HBM; nothing
here is timed by bench.py."""
from __future__ import annotations

import numpy as np

from . import demap as D


def noise_n0(constellation, rate, bps, ebn0_db):
    """N0 for Eb/N0 in dB with Es = mean |c|^2 (the 256QAM table is not
    unit-power: 1.0153, sdr_modem.py:195-207)."""
    es = float(np.mean(np.abs(np.asarray(constellation)) ** 2))
    return es / (rate * bps * 10 ** (ebn0_db / 10.0))


def make_symbols(codec, B, mod, ebn0_db, seed, device, cw0=0, want_info=True, fading=None, pilots=None, cfo=0.0,
                 tx=0, crc=None, streams=1):
    """(info uint8 [B, 2N] or None, received symbols complex64 [B, S], N0) on `device`.

    One launch of the counter-based generator (tdec_workload_dev): Philox info
    bits of GLOBAL codewords cw0 .. cw0+B-1 -> the LDS-staged encoder ->
    labelled Gray constellation (bps coded bits per label, MSB first, the last
    symbol zero-padded as the reference mappers pad, test_sdr_with_coding.py:45-86)
    -> complex AWGN with per-dimension variance N0/2.  Codeword g's data is the
    same whichever batch or rank generates it.

    fading={"K": Rician factor >= 0 (0: Rayleigh), "coh": symbols per gain block >= 1}:
    a flat-fading channel (tdec_workload_fading_dev), each symbol h x + n
    with the same bits and the same noise as without it, E|h|^2 = 1; the result is then
    (info, symbols, N0, h) with h complex64 [B, ceil(S / coh)].

    pilots=demap.PilotLayout(...) (with `fading`) frames those symbols with the layout's pilot blocks
    (tdec_workload_frame_dev): each pilot is h p + n with the gain of the data
    symbol it stands in front of and noise of the same variance from a stream of its own;
    cfo > 0 rotates frame position t of codeword g by exp(j 2 pi f_g t), f_g uniform in
    (-cfo, cfo) cycles per symbol per global codeword.  The result is then (info, frames, N0,
    h_true), frames and h_true complex64 [B, T], h_true the gain each position went through
    (rotation included); the data positions of a cfo = 0 frame are the unframed symbols.

    fading={..., "branches": R} (1 <= R <= 8): R independently faded,
    independently noisy copies of every codeword (tdec_workload_branches_dev, and
    tdec_workload_frame_branches_dev with `pilots`); symbols and gains, or frames and h_true,
    are then 3-D, [B, R, ...], branch 0 what the call without "branches" returns.  ebn0_db is
    per branch: the array gain is not charged.

    tx=t (1 .. 65535; hybrid ARQ): transmission t of the same codewords
    (harq_workload_tx_dev): the same info bits through `codec`'s pattern (a codec built
    with rv= sends another redundancy version), noise and gains of streams of their own,
    those of receive branch t.  With or without `fading`; neither `pilots` nor
    "branches".  tx=0 (default) is the calls above.

    crc="crc16" | "crc32" (DESIGN.md §16): the last r info bits of every codeword become the
    check field of the others (crc.attach_device on the counter-based info bits), and the
    generator encodes those bits (crc_workload_tx_dev): three launches on the codec's stream.
    The returned info bits carry the check field (they are always made; want_info only says
    whether they are returned); noise and gains are those of the same call without crc.  With
    `tx` and `fading`; neither `pilots` nor "branches".  crc=None (default) is the calls above.

    fading={..., "tx_antennas": 2}: the codeword is sent from two antennas with the
    Alamouti space-time block code (stbc_workload_dev) and received on "branches" (default 1)
    branches; "coh" counts slots and must be even.  The result is (info, slots complex64
    [B, R, S2], N0, h complex64 [B, R, 2, ceil(S2 / coh)]), S2 = S + (S & 1), 3-D / 4-D for one
    branch as well; h holds the effective gains, E|h|^2 = 1/2 each: the two antennas share the
    transmit power, so ebn0_db is per receive branch at fixed total transmit power.  Neither
    `pilots`, `tx` nor `crc`.  "tx_antennas" absent or 1 is the calls above.

    streams=2 (with `fading`): spatial multiplexing.  Slot m carries x[2m] from
    antenna 0 and x[2m+1] from antenna 1 (sm_workload_dev), received on "branches" (default 1)
    branches; "coh" counts slots, any value >= 1.  The result is (info, slots complex64 [B, R, T],
    N0, h complex64 [B, R, 2, ceil(T / coh)]), T = ceil(S / 2), the gains those of the Alamouti
    link (effective, E|h|^2 = 1/2 each), the silent antenna of an odd S sending 0.  Neither `pilots`,
    `tx`, `crc` nor "tx_antennas": 2.  streams=1 (default) is the calls above."""
    import torch
    from . import _native as _n
    if streams not in (1, 2) or isinstance(streams, bool):
        raise ValueError(f"streams must be 1 or 2, got {streams!r}")
    if streams == 2:
        if fading is None:
            raise ValueError("spatial multiplexing (streams = 2) needs a fading channel: pass fading={...}")
        if pilots is not None or tx or crc is not None or fading.get("tx_antennas", 1) == 2:
            raise ValueError("spatial multiplexing (streams = 2) takes neither pilots, tx, crc nor "
                             "fading['tx_antennas'] = 2")
        D.sm_order(mod)
    n_ant = 1 if fading is None else fading.get("tx_antennas", 1)
    if n_ant not in (1, 2) or isinstance(n_ant, bool):
        raise ValueError(f"fading: tx_antennas must be 1 or 2, got {n_ant!r}")
    if n_ant == 2:
        if pilots is not None or tx or crc is not None:
            raise ValueError("transmit diversity (tx_antennas = 2) takes neither pilots, tx nor crc")
        D.stbc_coh(fading.get("coh", 1))
        fading = {k: v for k, v in fading.items() if k != "tx_antennas"}
    elif fading is not None and "tx_antennas" in fading:   # 1: exactly the calls without the key
        fading = {k: v for k, v in fading.items() if k != "tx_antennas"}
    bps = D.MODULATIONS[mod]["bps"]
    cons = D.constellation(mod)
    rate = codec.k_info / codec.n_coded
    h = codec.handle
    S = -(-h.enc_len // bps)
    n0 = noise_n0(cons, rate, bps, ebn0_db)
    table = np.ascontiguousarray(cons.astype(np.complex64)).view(np.float32)
    info = torch.empty((B, codec.k_info), dtype=torch.uint8, device=device) if want_info else None
    if pilots is not None and fading is None:
        raise ValueError("pilots frames a fading channel's symbols: pass fading={...} as well")
    if pilots is None and cfo:
        raise ValueError("cfo needs pilots=PilotLayout(...)")
    cw0, seed, sigma = int(cw0), int(seed) & 0xFFFFFFFFFFFFFFFF, float(np.sqrt(n0 / 2))
    tx = int(tx)
    if tx:
        if not 0 < tx <= 65535:
            raise ValueError(f"tx must be 0 .. 65535, got {tx}")
        if pilots is not None or (fading is not None and fading.get("branches") is not None):
            raise ValueError("a retransmission (tx > 0) takes neither pilots nor receive branches")
    if crc is not None:
        return _make_symbols_crc(codec, B, crc, cw0, seed, table, len(cons), bps, sigma, n0, S, fading, pilots, tx,
                                 want_info, device)
    if fading is None and tx:
        syms = torch.empty((B, S), dtype=torch.complex64, device=device)
        h.call("harq_workload_tx_dev", int(B), tx, cw0, seed, _n.ptr(table), len(cons), bps, sigma, 0, 0.0, 1,
               _n.ptr(syms), None, _n.ptr(info), codec._stream(None))
        return info, syms, n0
    if fading is None:
        syms = torch.empty((B, S), dtype=torch.complex64, device=device)
        h.call("tdec_workload_dev", int(B), cw0, seed, _n.ptr(table), len(cons), bps, sigma, _n.ptr(syms),
               _n.ptr(info), codec._stream(None))
        return info, syms, n0
    unknown = set(fading) - {"K", "coh", "branches"}
    if unknown:
        raise ValueError(f"fading takes the keys 'K', 'coh' and 'branches', not {sorted(unknown)}")
    k, coh = float(fading.get("K", 0.0)), int(fading.get("coh", 1))
    if not (0.0 <= k < float("inf")) or coh < 1:
        raise ValueError("fading needs a finite K >= 0 and coh >= 1")
    R = fading.get("branches")
    if R is not None:
        R = int(R)
        if not 1 <= R <= D.MAX_BRANCHES:
            raise ValueError(f"fading: 1 .. {D.MAX_BRANCHES} branches, got {R}")
    if streams == 2:
        R, T = R or 1, (S + 1) // 2
        syms = torch.empty((B, R, T), dtype=torch.complex64, device=device)
        gains = torch.empty((B, R, 2, -(-T // coh)), dtype=torch.complex64, device=device)
        h.call("sm_workload_dev", int(B), R, cw0, seed, _n.ptr(table), len(cons), bps, sigma, k, coh, _n.ptr(syms),
               _n.ptr(gains), _n.ptr(info), codec._stream(None))
        return info, syms, n0, gains
    if n_ant == 2:
        R, S2 = R or 1, S + (S & 1)
        syms = torch.empty((B, R, S2), dtype=torch.complex64, device=device)
        gains = torch.empty((B, R, 2, -(-S2 // coh)), dtype=torch.complex64, device=device)
        h.call("stbc_workload_dev", int(B), R, cw0, seed, _n.ptr(table), len(cons), bps, sigma, k, coh, _n.ptr(syms),
               _n.ptr(gains), _n.ptr(info), codec._stream(None))
        return info, syms, n0, gains
    if pilots is not None:
        if not isinstance(pilots, D.PilotLayout):
            raise TypeError(f"pilots must be a demap.PilotLayout, got {type(pilots)}")
        if not (0.0 <= float(cfo) < float("inf")):
            raise ValueError("cfo must be a finite value >= 0")
    # R is None: 2-D results of the single-branch entry points; else [B, R, ...] of the branch ones (R behind B)
    rows, fade, frame = (((B,), "tdec_workload_fading_dev", "tdec_workload_frame_dev") if R is None else
                         ((B, R), "tdec_workload_branches_dev", "tdec_workload_frame_branches_dev"))
    syms = torch.empty((*rows, S), dtype=torch.complex64, device=device)
    gains = torch.empty((*rows, -(-S // coh)), dtype=torch.complex64, device=device)
    if tx:
        h.call("harq_workload_tx_dev", int(B), tx, cw0, seed, _n.ptr(table), len(cons), bps, sigma, 1, k, coh,
               _n.ptr(syms), _n.ptr(gains), _n.ptr(info), codec._stream(None))
        return info, syms, n0, gains
    h.call(fade, *map(int, rows), cw0, seed, _n.ptr(table), len(cons), bps, sigma, k, coh, _n.ptr(syms), _n.ptr(gains),
           _n.ptr(info), codec._stream(None))
    if pilots is None:
        return info, syms, n0, gains
    T = pilots.frame_len(S)
    frames = torch.empty((*rows, T), dtype=torch.complex64, device=device)
    h_true = torch.empty((*rows, T), dtype=torch.complex64, device=device)
    if B:
        _n.check(getattr(_n.lib(), frame)(
            h.device, _n.ptr(syms), _n.ptr(gains), *map(int, rows), S, coh, pilots.plen, pilots.dlen,
            _n.ptr(pilots.pilots_device(S, frames.device)), sigma, cw0, seed, float(cfo), _n.ptr(frames), _n.ptr(h_true),
            codec._stream(None)))
    return info, frames, n0, h_true


def _make_symbols_crc(codec, B, crc, cw0, seed, table, M, bps, sigma, n0, S, fading, pilots, tx, want_info, device):
    """make_symbols' crc= path: info bits -> check field -> the generator on those bits."""
    import torch
    from . import _native as _n
    from . import crc as CRC
    CRC.payload_bits(codec, crc)
    if pilots is not None or (fading is not None and fading.get("branches") is not None):
        raise ValueError("crc= takes neither pilots nor receive branches")
    k, coh = 0.0, 1
    if fading is not None:
        unknown = set(fading) - {"K", "coh", "branches"}
        if unknown:
            raise ValueError(f"fading takes the keys 'K', 'coh' and 'branches', not {sorted(unknown)}")
        k, coh = float(fading.get("K", 0.0)), int(fading.get("coh", 1))
        if not (0.0 <= k < float("inf")) or coh < 1:
            raise ValueError("fading needs a finite K >= 0 and coh >= 1")
    info = info_bits(codec, B, seed, device, cw0=cw0)
    if B:
        CRC.attach_device(info, crc, stream=codec._stream(None))
    syms = torch.empty((B, S), dtype=torch.complex64, device=device)
    gains = torch.empty((B, -(-S // coh)), dtype=torch.complex64, device=device) if fading is not None else None
    codec.handle.call("crc_workload_tx_dev", int(B), int(tx), cw0, seed, _n.ptr(table), M, bps, sigma,
                      int(fading is not None), k, coh, _n.ptr(info), _n.ptr(syms), _n.ptr(gains), codec._stream(None))
    info = info if want_info else None
    return (info, syms, n0) if fading is None else (info, syms, n0, gains)


def info_bits(codec, B, seed, device, cw0=0):
    """The info bits make_symbols encodes, uint8 [B, 2N]."""
    import torch
    info = torch.empty((B, codec.k_info), dtype=torch.uint8, device=device)
    codec.handle.call("tdec_info_bits_dev", int(B), int(cw0), int(seed) & 0xFFFFFFFFFFFFFFFF,
                      _ptr(info), codec._stream(None))
    return info


def count_errors(codec, bits, seed, cw0=0):
    """Bit errors per codeword (int32 [B]) of decoded rows against the
    counter-based info bits of global codewords cw0 .. cw0+B-1."""
    import torch
    B = bits.shape[0]
    if bits.dtype != torch.int32 or not bits.is_contiguous() or tuple(bits.shape) != (B, codec.k_info):
        raise ValueError("bits must be a contiguous int32 [B, 2N] tensor")
    errs = torch.empty(B, dtype=torch.int32, device=bits.device)
    codec.handle.call("tdec_count_errors_dev", int(B), int(cw0), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(bits),
                      _ptr(errs), codec._stream(None))
    return errs


def _ptr(t):
    from . import _native as _n
    return _n.ptr(t)


class DevicePipeline:
    """Demap -> turbo decode over device-resident symbols (the bench step).

    Default: the two launches k_demap_planes + k_turbo_decode over a plane
    buffer.  fused=True uses the one-launch k_turbo_decode_syms (each decoder
    wave demaps its next tile between the SISOs of the current one) where the
    handle has it; the bits are the same either way.  The fused launch measured
    3-4 % SLOWER on MI355X (294 vs 285 ms per 1 M codewords): a
    wave that demaps is not streaming, and at two waves per SIMD the decoder
    needs every wave streaming to keep HBM busy.  Buffers are sized once; run()
    is stream-ordered and allocation free.

    A codec built with early_stop=True decodes through the early-stop frame
    decoder, or with es_decoder="tile" / "refill" through the early-stop tile
    decoders (two launches, never fused; the codec's reserve() sizes what its
    decoder needs); the iterations each codeword of the last batch ran
    are in `n_iter` (int32 [B] on the device, first rows).

    demap="log-map" demaps with the exact log-sum demapper
    (tdec_demap_planes_logmap_dev) in front of either decoder algorithm; there
    is no fused kernel for it, so fused=True runs the two launches.

    run() also takes a per-row noise variance, a float64 [B] device tensor, on the
    two-launch and overlap paths; a pipeline built with fused=True
    refuses it, the fused kernel having no per-row form.

    csi=True sizes the equaliser's outputs (`z` complex64 [B, S], `nv_sym` float64 [B, S])
    so that run(..., csi=h, coh=...) equalises received symbols of a flat-fading channel
    with known gains and demaps them with a per-symbol noise variance:
    three launches on one stream; fused=True refuses it likewise.  run_frames() takes framed
    bursts with pilot blocks instead and estimates the gains (and, if asked, the noise
    variance) from them in the launch that equalises.

    Receive diversity: 3-D symbols [B, R, S] with csi [B, R, nh] go through
    the maximal-ratio combiner (demap.combine_device) in place of the equaliser, 3-D frames
    [B, R, T] through the pilot strip on all B * R rows and then the combiner; `z` and
    `nv_sym` are the same buffers, and everything behind them is unchanged.

    Transmit diversity: 4-D csi [B, R, 2, nh] with slots [B, R, S2] selects the
    Alamouti combiner (demap.stbc_combine_device) in place of the maximal-ratio one; it writes the
    same `z` and `nv_sym`, so there is nothing further to size and the call is allocation free from
    the first.  fused=True refuses it as it refuses csi, and run_frames refuses 4-D gains: pilot
    estimation for two transmit antennas is not built.

    llr="int8" | "f16"  models a soft-bit link between demapper and decoder: the
    flat demapper's LLRs (demap.compute_llr_device, decoder sign) are narrowed -- int8 by
    demap.quantize_llr_device with llr_step (default float32(30 / 127)), float16 by rounding -- into
    `llr_q`, and the narrow rows de-punctured into the planes (codec.depuncture_device).  The plane
    demappers have no flat LLRs: fused=True and overlap=True refuse it, as fused refuses csi.
    llr="f32" (default) is the pipeline above, unchanged.

    sm=True sizes one float32 [B, S * bps] buffer `llr_sm` for the joint detector of a
    spatially multiplexed 2 x R link, and run_sm(slots, noise_var, h, coh) runs detect
    (demap.sm_detect_device, decoder sign) -> the llr= narrowing, if any -> codec.depuncture_device ->
    decode.  The detector is max-log and has no plane form: fused=True, overlap=True and
    demap="log-map" are refused.  run() and run_frames() are untouched: with llr="int8" | "f16" the
    pipeline still holds the flat demapper's float64 buffer `llr`, which run() narrows from and
    run_sm() (its LLRs are float32 already) does not use."""

    def __init__(self, codec, mod, B, device, fused=False, overlap=False, gate=True, demap="max-log", csi=False,
                 llr="f32", llr_step=None, sm=False):
        import torch
        self.codec, self.mod, self.B = codec, mod, B
        self.llr_kind, self.llr_step = _llr_link(llr, llr_step)
        self.sm = bool(sm)
        if self.sm:
            if fused or overlap or demap != "max-log":
                raise ValueError("sm=True detects jointly into flat max-log LLRs: it takes neither fused=True, "
                                 "overlap=True nor demap='log-map'")
            D.sm_order(mod)
        if self.llr_kind is not None and (fused or overlap):
            raise ValueError(f"llr={llr!r} needs the flat demapper's LLRs: the plane demappers of fused=True and "
                             "overlap=True have none")
        self.bps = D.MODULATIONS[mod]["bps"]
        self.cons = D.constellation(mod)
        self.demap = demap
        lm = D.check_algo(demap)
        # the division's dtype when the noise variance is a tensor: what a numpy float64 scalar gives
        self.div_f32_t = D.demap_mode(np.complex64, self.cons.dtype, np.float64(1.0))[1]
        self.early_stop = bool(getattr(codec, "early_stop", False))
        self.fused_asked = bool(fused)
        self.fused = (bool(fused) and not lm and not self.early_stop
                      and codec.fused_available(self.cons, self.bps))
        self.overlap = bool(overlap) and not self.fused
        if self.fused:
            codec.reserve_fused(B)
            self.planes = None
        else:
            codec.reserve(B)
            self.planes = torch.empty(codec.planes_bytes(B) // 4, dtype=torch.float32, device=device)
        self.bits = torch.empty((B, codec.k_info), dtype=torch.int32, device=device)
        self.n_iter = torch.empty(B, dtype=torch.int32, device=device) if self.early_stop else None
        self.llr = self.llr_q = None
        if self.llr_kind is not None:
            self.llr, self.llr_q = _llr_link_buffers(self.llr_kind, B * -(-codec.handle.enc_len // self.bps) * self.bps,
                                                     device)
        self.llr_sm = None
        if self.sm:
            self.llr_sm = torch.empty((B, -(-codec.handle.enc_len // self.bps) * self.bps), dtype=torch.float32,
                                      device=device)
        self.z = self.nv_sym = None
        self._strip = {}                          # run_frames' per-branch buffers, by R (sized on first use)
        if csi:
            S = -(-codec.handle.enc_len // self.bps)
            self.z = torch.empty((B, S), dtype=torch.complex64, device=device)
            self.nv_sym = torch.empty((B, S), dtype=torch.float64, device=device)
        if self.overlap:
            # Batch i+1's demap runs on its own handle (handles order only their own
            # buffers), its own low-priority stream and the other plane buffer, so
            # it can start as soon as batch i's persistent decoder waves begin to
            # retire (tail of the persistent launch) instead of after
            # the last one.  The decode runs on a high-priority stream, so a decode
            # and a demap that become ready together dispatch the decode first.
            import copy
            self.demapper = copy.copy(codec)
            self.demapper._h = None
            self.planes_db = [self.planes, torch.empty_like(self.planes)]
            self.s_demap = torch.cuda.Stream(device=device, priority=0)
            self.s_decode = torch.cuda.Stream(device=device, priority=-1)
            self.demap_done = [torch.cuda.Event(), torch.cuda.Event()]
            self.decode_done = [torch.cuda.Event(), torch.cuda.Event()]
            self.step = 0
            self.gate = bool(gate)

    def run(self, syms, noise_var, stream=None, events=None, syms_ready=None, csi=None, coh=1):
        """One batch: demap -> decode, stream-ordered on `stream` (its bits are ready
        for work queued on `stream` afterwards).  With overlap=True, `syms_ready`
        (an event after which `syms` is valid) lets the demap start before the
        previous batch's decode has finished; without it the demap waits for
        everything queued on `stream`, i.e. no overlap.

        noise_var: a scalar, or a float64 [B] tensor on the symbols' device with one
        value per row (demap.estimate_noise_var_device queued on the same stream
        gives it), which the demapper reads on the device.

        csi: the channel gains of `syms`, complex64 [B, ceil(S / coh)] on their device
        (symbol s of a row was received through csi[:, s // coh]); the symbols are
        equalised into `z` and demapped with `nv_sym` = noise_var / |csi|^2 per symbol.
        Needs a pipeline built with csi=True.

        3-D `syms` [B, R, S] (with csi [B, R, nh]) are R receive branches of each burst: the
        combiner takes the equaliser's place; noise_var may then also be a float64 [B, R]
        tensor, one value per branch."""
        if syms.dim() == 3 and csi is None:
            raise ValueError("3-D symbols are receive branches: they need their gains (csi=h)")
        if csi is not None and csi.dim() == 4:
            return self._run_stbc(syms, noise_var, stream, events, syms_ready, csi, coh)
        if csi is not None:
            if self.fused_asked:
                raise ValueError("csi needs the two-launch pipeline: the fused demap+decode kernel has no "
                                 "per-symbol form (fused=True)")
            if self.z is None:
                raise ValueError("csi needs a pipeline built with csi=True")
            if syms.shape[0] > self.B or syms.shape[-1] != self.z.shape[1]:
                raise ValueError(f"csi: symbols must be [<= {self.B}, {self.z.shape[1]}] or [<= {self.B}, R, "
                                 f"{self.z.shape[1]}], got {tuple(syms.shape)}")
        front = None
        if csi is not None and syms.dim() == 3:
            front = lambda st: self._front(D.combine_device, syms, csi, noise_var, coh, st)  # noqa: E731
            return self._run(syms, 1.0, stream, events, syms_ready, front)
        if csi is not None:
            front = lambda st: self._front(D.equalize_device, syms, csi, noise_var, coh, st)  # noqa: E731
        return self._run(syms, noise_var, stream, events, syms_ready, front)

    def run_sm(self, y, noise_var, h, coh=1, stream=None, events=None):
        """One batch of a spatially multiplexed link: slots complex64 [n <= B, R, T],
        T = ceil(S / 2), with the known effective gains h complex64 [n, R, 2, ceil(T / coh)] -> the joint
        detector's decoder-sign LLRs into `llr_sm` -> (llr="int8" | "f16": narrowed into `llr_q`) ->
        the de-puncture kernel -> the decode, all on `stream`.  noise_var: a scalar, a float64 [n] or a
        float64 [n, R] device tensor.  Allocation free; returns the bits (a view of `bits`), and with
        an early-stop codec `n_iter` holds the iterations, as after run()."""
        import torch
        if not self.sm:
            raise ValueError("run_sm needs a pipeline built with sm=True")
        L = self.llr_sm.shape[1]
        S = L // self.bps
        if not isinstance(y, torch.Tensor) or y.dim() != 3 or y.shape[0] > self.B or y.shape[2] != (S + 1) // 2:
            raise ValueError(f"the slots must be [<= {self.B}, R, {(S + 1) // 2}], got {tuple(getattr(y, 'shape', ()))}")
        n = y.shape[0]
        llr = D.sm_detect_device(y, h, self.mod, noise_var, S=S, coh=coh, out=self.llr_sm[:n], sign=-1, stream=stream)
        if self.llr_kind == "int8":
            q = self.llr_q[:n * L].view(n, L)
            D.quantize_llr_device(llr, self.llr_step, out=q, stream=stream)
            llr = q
        elif self.llr_kind == "f16":
            q = self.llr_q[:n * L].view(n, L)
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(y.device)):
                q.copy_(llr)   # float32 -> float16, round to nearest even
            llr = q
        self.codec.depuncture_device(llr, self.planes, stream=stream, llr_step=self.llr_step)
        if events is not None:
            events[0].record(stream)
        bits = self.bits[:n]
        es = {"n_iter": self.n_iter[:n]} if self.early_stop else {}
        self.codec.decode_planes_device(self.planes, n, bits, stream=stream, **es)
        if events is not None:
            events[1].record(stream)
        return bits

    def _run_stbc(self, syms, noise_var, stream, events, syms_ready, csi, coh):
        """run() for an Alamouti link: slots [n, R, S2] with 4-D gains [n, R, 2, nh] through
        demap.stbc_combine_device into `z` / `nv_sym`; everything behind them is unchanged."""
        if self.fused_asked:
            raise ValueError("csi needs the two-launch pipeline: the fused demap+decode kernel has no "
                             "per-symbol form (fused=True)")
        if self.z is None:
            raise ValueError("csi needs a pipeline built with csi=True")
        S = self.z.shape[1]
        if syms.dim() != 3 or syms.shape[0] > self.B or syms.shape[2] != S + (S & 1):
            raise ValueError(f"4-D gains are two transmit antennas': the slots must be [<= {self.B}, R, {S + (S & 1)}], "
                             f"got {tuple(syms.shape)}")
        coh = D.stbc_coh(coh)
        n = syms.shape[0]

        def front(st):
            z, nvs = D.stbc_combine_device(syms, csi, noise_var, S=S, coh=coh, out=self.z[:n], nv_out=self.nv_sym[:n],
                                           stream=st)
            return z, nvs, self.div_f32_t
        return self._run(syms, 1.0, stream, events, syms_ready, front)

    def run_frames(self, frames, layout, noise_var=None, mode="linear", stream=None, events=None, csi=None):
        """One batch of framed bursts (demap.PilotLayout): the pilots' channel
        estimate and the equalisation in one launch into `z` / `nv_sym`, the per-symbol
        demap, the decode, all on `stream`.  noise_var: a scalar, a float64 [B] device
        tensor, or None: each burst's own estimate from its pilots (plen >= 2).  Needs a
        pipeline built with csi=True; fused=True refuses it as it refuses csi.

        3-D `frames` [B, R, T] are R receive branches of each burst: one strip
        launch over the B * R rows (stripped data, interpolated gains and, for noise_var None,
        each branch's own noise estimate), then the combiner; an estimated noise goes in per
        branch, a scalar or [B] noise_var as the common one.

        csi: refused.  run_frames estimates the gains from the pilots, and for the 4-D gains of two
        transmit antennas no pilot layout or estimator is built: run() takes those."""
        if (csi is not None and csi.dim() == 4) or frames.dim() == 4:
            raise ValueError("run_frames has no pilot estimation for two transmit antennas (4-D gains): pass the "
                             "known gains to run(slots, nv, csi=h, coh=...)")
        if csi is not None:
            raise ValueError("run_frames estimates the gains from the pilots: it takes no csi")
        if self.fused_asked:
            raise ValueError("framed bursts need the two-launch pipeline: the fused demap+decode kernel has no "
                             "per-symbol form (fused=True)")
        if self.z is None:
            raise ValueError("run_frames needs a pipeline built with csi=True")
        S = self.z.shape[1]
        if frames.dim() == 3:
            return self._run_branch_frames(frames, layout, noise_var, mode, stream, events)
        if frames.dim() != 2 or frames.shape[0] > self.B or frames.shape[1] != layout.frame_len(S):
            raise ValueError(f"frames must be [<= {self.B}, {layout.frame_len(S)}], got {tuple(frames.shape)}")
        n = frames.shape[0]

        def front(st):
            z, nvs = D.estimate_csi_device(frames, layout, noise_var, mode=mode, out=self.z[:n],
                                           nv_out=self.nv_sym[:n], stream=st)
            return z, nvs, self.div_f32_t
        return self._run(frames, 1.0, stream, events, None, front)

    def _run_branch_frames(self, frames, layout, noise_var, mode, stream, events):
        """run_frames for [B, R, T]: strip on B * R rows, then combine."""
        import torch
        S = self.z.shape[1]
        n, R, T = frames.shape
        if n > self.B or not 1 <= R <= D.MAX_BRANCHES or T != layout.frame_len(S):
            raise ValueError(f"frames must be [<= {self.B}, 1 .. {D.MAX_BRANCHES}, {layout.frame_len(S)}], "
                             f"got {tuple(frames.shape)}")
        if not frames.is_contiguous():
            raise ValueError("frames must be a contiguous tensor on a HIP device")
        if R not in self._strip:
            dev = self.z.device
            self._strip[R] = (torch.empty((self.B * R, S), dtype=torch.complex64, device=dev),
                              torch.empty((self.B * R, S), dtype=torch.complex64, device=dev),
                              torch.empty(self.B * R, dtype=torch.float64, device=dev))
        y, h, nvb = (t[:n * R] for t in self._strip[R])
        estimate = noise_var is None

        def front(st):
            D.strip_pilots_device(frames.view(n * R, T), layout, mode=mode, out=y, h_out=h,
                                  nv_rows_out=nvb if estimate else None, stream=st)
            return self._front(D.combine_device, y.view(n, R, S), h.view(n, R, S),
                               nvb.view(n, R) if estimate else noise_var, 1, st)
        return self._run(frames, 1.0, stream, events, None, front)

    def _run(self, syms, noise_var, stream, events, syms_ready, front):
        """run()'s launches.  front (optional): queues what stands in front of the demapper on
        the stream it is given and returns (symbols, noise variance, div_f32) for it."""
        import torch
        if isinstance(noise_var, torch.Tensor):
            if self.fused_asked:
                raise ValueError("a per-row noise_var tensor needs the two-launch pipeline: the fused "
                                 "demap+decode kernel has no per-row form (fused=True)")
            div32, nve = self.div_f32_t, noise_var
        else:
            _, div32, nve = D.demap_mode(np.complex64, self.cons.dtype, np.float64(noise_var))
        bits = self.bits[:syms.shape[0]]          # the first rows: a contiguous view
        es = {"n_iter": self.n_iter[:syms.shape[0]]} if self.early_stop else {}
        if self.overlap:
            stream = torch.cuda.current_stream() if stream is None else stream
            b = self.step & 1
            sd, sk = self.s_demap, self.s_decode
            if self.step >= 2:
                sd.wait_event(self.decode_done[b])      # planes[b]'s last reader (batch i-2)
            if syms_ready is not None:
                sd.wait_event(syms_ready)
            else:
                sd.wait_stream(stream)
            if self.gate:
                self.codec.tail_gate(sd)                # batch i-1's decode is in its tail
            if front is not None:
                syms, nve, div32 = front(sd)
            self.demapper.demap_planes_device(syms, self.cons, self.bps, nve, self.planes_db[b], div_f32=div32,
                                              stream=sd, algo=self.demap)
            self.demap_done[b].record(sd)
            sk.wait_stream(stream)                      # earlier readers of bits on the caller's stream
            sk.wait_event(self.demap_done[b])
            if events is not None:
                events[0].record(sk)
            self.codec.decode_planes_device(self.planes_db[b], syms.shape[0], bits, stream=sk, **es)
            if events is not None:
                events[1].record(sk)
            self.decode_done[b].record(sk)
            stream.wait_event(self.decode_done[b])
            self.step += 1
            return bits
        if self.fused:
            if events is not None:
                events[0].record(stream)
            self.codec.demap_decode_device(syms, self.cons, self.bps, nve, bits, div_f32=div32, stream=stream)
        else:
            if front is not None:
                syms, nve, div32 = front(stream)
            if self.llr_kind is not None:
                n, L = syms.shape[0], syms.shape[1] * self.bps
                q = _llr_link_run(self, syms, nve if isinstance(nve, torch.Tensor) else np.float64(noise_var), n, L, stream)
                self.codec.depuncture_device(q, self.planes, stream=stream, llr_step=self.llr_step)
            else:
                self.codec.demap_planes_device(syms, self.cons, self.bps, nve, self.planes, div_f32=div32,
                                               stream=stream, algo=self.demap)
            if events is not None:
                events[0].record(stream)
            self.codec.decode_planes_device(self.planes, syms.shape[0], bits, stream=stream, **es)
        if events is not None:
            events[1].record(stream)
        return bits

    def _front(self, fn, syms, csi, nv, coh, stream):
        """(z, nv_sym, div_f32) for the demapper: `syms` equalised by `csi` (fn = demap.equalize_device)
        or its [B, R, S] receive branches combined (demap.combine_device) into this pipeline's buffers
        on `stream` (nv unfloored: the demapper floors nv / |h|^2); the division's dtype is the
        tensor forms'."""
        n = syms.shape[0]
        z, nvs = fn(syms, csi, nv, coh=coh, out=self.z[:n], nv_out=self.nv_sym[:n], stream=stream)
        return z, nvs, self.div_f32_t


def _llr_link(llr, llr_step):
    """(kind, step) of a pipeline's llr= / llr_step= arguments: (None, None) for "f32", else
    ('int8' | 'f16', the int8 step or None); llr_step with anything but int8 is a TypeError."""
    from .dvb_rcs2_turbo import llr_step_arg
    if llr not in ("f32", "int8", "f16"):
        raise ValueError(f"unknown llr {llr!r} ('f32', 'int8' or 'f16')")
    if llr != "int8" and llr_step is not None:
        raise TypeError("llr_step applies to llr='int8' only")
    if llr == "f32":
        return None, None
    return llr, (llr_step_arg(llr, llr_step) if llr == "int8" else None)


def _llr_link_buffers(kind, n, device):
    """The flat demapper's float64 LLRs and their narrow form, n elements each."""
    import torch
    return (torch.empty(n, dtype=torch.float64, device=device),
            torch.empty(n, dtype=torch.int8 if kind == "int8" else torch.float16, device=device))


def _llr_link_run(p, syms, nv, n, L, stream):
    """Flat demap of `syms` (decoder sign) into p.llr, narrowed into p.llr_q: the [n, L] narrow rows."""
    import torch
    llr, q = p.llr[:n * L].view(n, L), p.llr_q[:n * L].view(n, L)
    D.compute_llr_device(syms, p.mod, nv, out=llr, sign=-1, stream=stream, algo=p.demap)
    if p.llr_kind == "int8":
        D.quantize_llr_device(llr, p.llr_step, out=q, stream=stream)
    else:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(syms.device)):
            q.copy_(llr)   # float64 -> float16, round to nearest even (one rounding)
    return q


class HarqPipeline:
    """Hybrid ARQ receiver: every transmission of a batch of codewords is
    soft-combined into one plane buffer, which `mother`'s decoder reads after each.

    codecs: the codec of each transmission, cycled (transmission t uses codecs[t % len]).
    Chase combining is [c]; incremental redundancy is
    [DVBRCS2_Turbo(N, rate, rv=r, ...) for r in range(period)].  mother: the codec whose
    decoder reads the combined planes -- for Chase the same codec, for incremental
    redundancy a rate-1/3 codec of the same N, interleaver and inv_perm (its early_stop /
    es_decoder / algo choose the decoder).  A codec whose N, perm or inv_perm differs from
    mother's is refused: the planes would mean something else to the decoder.

    receive(t, syms, noise_var, active=None) queues, on one stream and with no host round
    trip: transmission 0 through codecs[0]'s fused plane demapper straight into the planes;
    transmission t > 0 through the flat demapper (demap.compute_llr_device, decoder sign) and
    the combining kernel (depuncture_accumulate_device); then mother.decode_planes_device.
    max_tx bounds t.  Buffers are sized once.

    crc="crc16" | "crc32" (DESIGN.md §16): the codewords carry a check field
    (make_symbols(..., crc=...)).  After every decode the bits are verified on the device into
    `ack` (int32 [B]: 1 = the row passed), and a receive(t > 0) without `active` combines only
    the rows whose ack is 0 from the call before: the retransmission loop runs with no host
    decision in it.  An explicit `active` still wins.  crc=None: no `ack`, nothing else changes.

    llr="int8" | "f16" (llr_step: int8's step): every transmission, the first
    included, goes through the flat demapper, is narrowed as DevicePipeline narrows it and is
    de-punctured (t = 0) or combined (t > 0) from the narrow rows."""

    def __init__(self, codecs, mother, mod, B, device, demap="max-log", max_tx=4, crc=None, llr="f32", llr_step=None):
        import torch
        self.llr_kind, self.llr_step = _llr_link(llr, llr_step)
        codecs = list(codecs)
        if not codecs:
            raise ValueError("HarqPipeline needs at least one transmission codec")
        for i, c in enumerate(codecs):
            if c.N != mother.N or not np.array_equal(c.perm, mother.perm) or not np.array_equal(c.inv_perm, mother.inv_perm):
                raise ValueError(f"codecs[{i}] and mother differ in N, perm or inv_perm: their planes are not "
                                 "the same code's")
            if c.device != mother.device:
                raise ValueError(f"codecs[{i}] and mother are on different devices")
        if int(max_tx) < 1:
            raise ValueError("max_tx must be >= 1")
        self.codecs, self.mother, self.mod, self.B, self.max_tx = codecs, mother, mod, int(B), int(max_tx)
        self.bps = D.MODULATIONS[mod]["bps"]
        self.cons = D.constellation(mod)
        self.demap = demap
        D.check_algo(demap)
        self.div_f32_t = D.demap_mode(np.complex64, self.cons.dtype, np.float64(1.0))[1]
        self.early_stop = bool(getattr(mother, "early_stop", False))
        mother.reserve(self.B)
        self.planes = torch.empty(mother.planes_bytes(self.B) // 4, dtype=torch.float32, device=device)
        self.bits = torch.empty((self.B, mother.k_info), dtype=torch.int32, device=device)
        self.n_iter = torch.empty(self.B, dtype=torch.int32, device=device) if self.early_stop else None
        # symbols per codeword of each transmission codec (the versions of one rate differ where N % period != 0)
        self.S = [-(-c.handle.enc_len // self.bps) for c in codecs]
        self.llr = torch.empty(self.B * max(self.S) * self.bps, dtype=torch.float64, device=device)
        self.llr_q = None
        if self.llr_kind is not None:
            self.llr_q = _llr_link_buffers(self.llr_kind, self.llr.numel(), device)[1]
        self.row_of = torch.empty(self.B, dtype=torch.int32, device=device)
        self._iota = torch.arange(self.B, dtype=torch.int32, device=device)
        self._none = torch.full((self.B,), -1, dtype=torch.int32, device=device)
        self.crc, self.ack = crc, None
        if crc is not None:
            from . import crc as CRC
            CRC.payload_bits(mother, crc)
            self.bits.zero_()
            # (the first check of a row length uploads its table: here, not between transmissions)
            self.ack = CRC.check_device(self.bits, crc) if self.B else torch.zeros(0, dtype=torch.int32, device=device)
            self.ack.zero_()

    def codec(self, t):
        """The codec transmission t is sent with."""
        return self.codecs[t % len(self.codecs)]

    def receive(self, t, syms, noise_var, active=None, stream=None):
        """Transmission t (0 .. max_tx - 1) of the batch: complex64 [n <= B, S_t] device symbols,
        S_t the symbols of codec(t); equalised ones (demap.equalize_device's z) for a fading
        channel.  noise_var: a scalar, a float64 [n] device tensor (one per row) or a
        float64 [n, S_t] one (one per symbol, equalize_device's nv_sym).  active (t > 0): a bool
        or int32 [n] device tensor; rows with 0 are not combined, so their planes and hence
        their bits stay as they were (None: every row, or with crc= the rows whose `ack` is 0).
        Returns the bits, int32 [n, 2N] (a view of `bits`), ready for work queued on `stream`
        afterwards; with crc=, `ack[:n]` is their frame check."""
        import torch
        t = int(t)
        if not 0 <= t < self.max_tx:
            raise ValueError(f"transmission {t} outside 0 .. {self.max_tx - 1} (max_tx)")
        c, S = self.codec(t), self.S[t % len(self.codecs)]
        if not isinstance(syms, torch.Tensor) or syms.dim() != 2 or syms.shape[0] > self.B or syms.shape[1] != S:
            raise ValueError(f"transmission {t}: symbols must be [<= {self.B}, {S}], got "
                             f"{tuple(getattr(syms, 'shape', ()))}")
        n = syms.shape[0]
        if isinstance(noise_var, torch.Tensor):
            div32, nve = self.div_f32_t, noise_var
        else:
            _, div32, nve = D.demap_mode(np.complex64, self.cons.dtype, np.float64(noise_var))
        nvf = nve if isinstance(nve, torch.Tensor) else np.float64(noise_var)   # the flat demapper's
        if t == 0:
            if active is not None:
                raise ValueError("transmission 0 writes every row's planes: it takes no `active`")
            if self.llr_kind is not None:
                c.depuncture_device(_llr_link_run(self, syms, nvf, n, S * self.bps, stream), self.planes, stream=stream,
                                    llr_step=self.llr_step)
            else:
                c.demap_planes_device(syms, self.cons, self.bps, nve, self.planes, div_f32=div32, stream=stream,
                                      algo=self.demap)
        else:
            row_of = None
            if active is not None:
                if (not isinstance(active, torch.Tensor) or active.dtype not in (torch.bool, torch.int32)
                        or tuple(active.shape) != (n,) or active.device != self.row_of.device):
                    raise ValueError(f"active must be a bool or int32 [{n}] tensor on the pipeline's device")
                row_of = self.row_of[:n]
                with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(c.device)):
                    torch.where(active != 0, self._iota[:n], self._none[:n], out=row_of)
            elif self.crc is not None:   # the rows the previous call's frame check failed
                row_of = self.row_of[:n]
                with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(c.device)):
                    torch.where(self.ack[:n] == 0, self._iota[:n], self._none[:n], out=row_of)
            if self.llr_kind is not None:
                c.depuncture_accumulate_device(_llr_link_run(self, syms, nvf, n, S * self.bps, stream), self.planes, n,
                                               row_of=row_of, stream=stream, llr_step=self.llr_step,
                                               f16=self.llr_kind == "f16")
            else:
                llr = self.llr[:n * S * self.bps].view(n, S * self.bps)
                # (a numpy float64 scalar: the division's dtype of transmission 0's plane demapper)
                D.compute_llr_device(syms, self.mod, nvf, out=llr, sign=-1, stream=stream, algo=self.demap)
                c.depuncture_accumulate_device(llr, self.planes, n, row_of=row_of, stream=stream)
        bits = self.bits[:n]
        es = {"n_iter": self.n_iter[:n]} if self.early_stop else {}
        self.mother.decode_planes_device(self.planes, n, bits, stream=stream, **es)
        if self.crc is not None:
            from . import crc as CRC
            CRC.check_device(bits, self.crc, ok=self.ack[:n], stream=stream)
        return bits
