#!/usr/bin/env python3
"""Generate tests/golden/decode_matrix.npz: the reference's decode() on every
codec of its tables, INTERLEAVER_PARAMS x PUNCTURE_PATTERNS (7 block sizes x
4 rates = 28).

TEST INFRASTRUCTURE ONLY, built like make_golden.py and run where that runs:
the reference module is imported unmodified through make_golden.py's numba
stand-in, and only inputs and recorded outputs (no code) are written.

Per codec, keyed ``<name>_<N>_<num>_<den>``:

  info    int32 [2, 2N]      the information bits
  coded   int32 [2, n_enc]   encode(info), at encode()'s own length
  llr     float32 [2, walk]  QPSK-over-AWGN LLRs of ``coded`` at Eb/N0 = 1 dB
                             (row 0) and 3 dB (row 1), zero-padded to the
                             de-puncture walk of decode() (:476-487) where
                             encode() or n_coded is shorter (the period does
                             not divide N: rate 2/3 at every N but 48)
  bits    int32 [2, 2N]      decode(llr)
  lfinal  float64 [2, 2N]    Lc + La + Le1 of the final decision (:529-530)
  inv     int32 [N]          np.argsort(perm, kind="stable"), the inverse
                             interleaver the decodes ran with

The file is written with fixed archive timestamps, so a re-run reproduces it
byte for byte.

Usage:  python tests/golden/make_golden_matrix.py   (about two minutes)
"""
import io
import os
import sys
import time
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

from make_golden import _decode_capture, _import_reference, _qpsk_llrs, make_codec  # noqa: E402

EBN0_DB = (1.0, 3.0)


def _walk(c):
    """LLRs decode()'s de-puncture loop reads (:476-487)."""
    p, per = c.punct, c.punct["period"]
    return sum(2 + p["W1"][i % per] + p["Y1"][i % per] + p["W2"][i % per] + p["Y2"][i % per] for i in range(c.N))


def save_npz(path, arrays):
    """np.savez_compressed with the archive members' timestamps fixed."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def gen_decode_matrix(T):
    out = {}
    for n in T.INTERLEAVER_PARAMS:
        for rate in T.PUNCTURE_PATTERNS:
            num, den = (int(x) for x in rate.split("/"))
            c = make_codec(T, n, rate)
            c.inv_perm = np.argsort(c.perm, kind="stable").astype(np.int32)
            rng = np.random.default_rng([20261020, n, num, den])
            walk = _walk(c)
            rows = []
            for e in EBN0_DB:
                info = rng.integers(0, 2, c.k_info).astype(np.int32)
                coded = c.encode(info)
                # QPSK carries two bits a symbol: an odd codeword (rate 3/4 at N = 212) gets one
                # filler bit for the last symbol, whose LLR is dropped again
                llr = _qpsk_llrs(rng, np.append(coded, 0) if len(coded) % 2 else coded, e, num / den)[:len(coded)]
                if len(llr) < walk:
                    llr = np.pad(llr, (0, walk - len(llr)))
                t = time.time()
                bits, lf = _decode_capture(T, c, llr)
                print(f"  decode N={n} r={rate} ebn0={e} errs={int((bits != info).sum())} "
                      f"({time.time() - t:.1f}s)", flush=True)
                rows.append((info, coded, llr, bits, lf))
            key = f"{n}_{num}_{den}"
            for name, col in zip(("info", "coded", "llr", "bits", "lfinal"), zip(*rows)):
                out[f"{name}_{key}"] = np.stack(col)
            out[f"inv_{key}"] = c.inv_perm
    save_npz(os.path.join(OUT, "decode_matrix.npz"), out)


if __name__ == "__main__":
    gen_decode_matrix(_import_reference())
