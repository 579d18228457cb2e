"""The frame check's restatement (tests/crc_ref.py) against the known
answers, and the C ABI's bookkeeping.  No GPU."""
import binascii
import os
import re

import numpy as np
import pytest

import crc_ref as R
from modulations_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("crc16", "crc32")
# every row length the GPU tests use: r + 8, 96, 424, 1504, 1696, 2048
LENGTHS = {k: (R.KINDS[k][0] + 8, 96, 424, 1504, 1696, 2048) for k in KINDS}


def _bitrev(v, n):
    return int(format(v, f"0{n}b")[::-1], 2)


def _strings():
    rng = np.random.default_rng(16)
    return [b"123456789"] + [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (8, 12, 94, 188)]


def test_known_answers():
    bits = R.bytes_to_bits(b"123456789")
    assert int(R.register(bits, "crc16")[0]) == 0x29B1
    assert int(R.register(bits, "crc32")[0]) == 0x0376E6E7


@pytest.mark.parametrize("data", _strings(), ids=lambda d: f"{len(d)}B")
def test_binascii_identities(data):
    bits = R.bytes_to_bits(data)
    assert int(R.register(bits, "crc16")[0]) == binascii.crc_hqx(data, 0xFFFF)
    reflected = bytes(_bitrev(b, 8) for b in data)
    assert int(R.register(bits, "crc32")[0]) == _bitrev(binascii.crc32(reflected), 32) ^ 0xFFFFFFFF


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("data", _strings(), ids=lambda d: f"{len(d)}B")
def test_residue_is_zero_after_attach(kind, data):
    r = R.KINDS[kind][0]
    row = np.concatenate([R.bytes_to_bits(data), np.zeros(r, np.uint8)])
    full = R.attach(row, kind)
    assert np.array_equal(full[0, :-r], row[:-r])
    reg = int(R.register(row[:-r], kind)[0])
    assert "".join(map(str, full[0, -r:])) == format(reg, f"0{r}b")            # the register, MSB first
    assert int(R.remainder(full, kind)[0]) == 0
    full[0, 3] ^= 1
    assert int(R.remainder(full, kind)[0]) != 0


@pytest.mark.parametrize("kind", KINDS)
def test_affine_form_equals_the_register_loop(kind):
    rng = np.random.default_rng(R.KINDS[kind][0])
    for L in LENGTHS[kind]:
        rows = rng.integers(0, 2, (5, L)).astype(np.int32)
        rows[0], rows[1] = 0, 1
        rows[2] = R.attach(rows[2], kind)[0]
        rows[3] = rows[3] * 2 + rng.integers(0, 2, L) - 2 * rng.integers(0, 2, L)   # only bit 0 counts
        want = R.remainder(rows, kind)
        assert np.array_equal(R.remainder_affine(rows, kind), want), L
        assert want[2] == 0 and want[0] != 0
        T, c = R.table(kind, L)
        assert int(c) == int(R.register(np.zeros(L, np.uint8), kind)[0])           # the all-zero row's register
        assert int(T[L - 1]) == R.KINDS[kind][1]                                   # x^r mod g


def test_only_bit_zero_of_an_element_counts():
    rng = np.random.default_rng(2)
    bits = rng.integers(0, 2, (3, 96)).astype(np.int32)
    for kind in KINDS:
        want = R.remainder(bits, kind)
        assert np.array_equal(R.remainder(bits + 2, kind), want)
        assert np.array_equal(R.remainder(-bits, kind), want)                      # -1 is a set bit
        assert np.array_equal(R.remainder(bits.astype(np.uint8), kind), want)


# ---- the C ABI's bookkeeping ---------------------------------------------------------------

def _crc_header_symbols():
    src = open(os.path.join(ROOT, "include", "crc.h")).read()
    return sorted(set(re.findall(r"^\s*(?:[\w\s\*]+?)\b(crc_\w+)\s*\(", src, re.M)))


def test_crc_header_matches_binding_list():
    assert _crc_header_symbols() == sorted(_native.CRC_EXPORTS)
    assert not set(_native.CRC_EXPORTS) & (set(_native.EXPORTS) | set(_native.HARQ_EXPORTS))
    src = open(os.path.join(ROOT, "include", "crc.h")).read()
    for kind, (r, _, _) in R.KINDS.items():
        assert _native.CRC_KINDS[kind] == r
        assert re.search(rf"#define CRC_KIND{r} {r}\b", src)


def test_python_constants_match_the_header():
    from modulations_amd import crc
    src = open(os.path.join(ROOT, "include", "crc.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (CRC_\w+) (\d+)", src)}
    assert crc.GRID_ROWS == d["CRC_MAX_BLOCKS"] * d["CRC_ROWS_PER_BLOCK"]
    assert crc.MAX_ROW_BITS == d["CRC_MAX_ROW_BITS"]
    assert {k: (v["r"], v["poly"], v["init"]) for k, v in crc.KINDS.items()} == R.KINDS


def test_library_exports_the_crc_symbols():
    import ctypes as C
    import subprocess
    lib = _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    for name in _native.CRC_EXPORTS:
        assert re.search(rf"\bT {name}$", out, re.M), name
        assert getattr(lib, name).restype is C.c_int
    assert [a.__name__ for a in lib.crc_check_dev.argtypes] == \
        ["c_int", "c_int", "c_long", "c_int", "c_void_p", "c_void_p", "c_void_p", "c_void_p"]
    assert [a.__name__ for a in lib.crc_workload_tx_dev.argtypes] == \
        ["c_void_p", "c_int", "c_int", "c_long", "c_ulong", "c_void_p", "c_int", "c_int", "c_double", "c_int",
         "c_double", "c_int", "c_void_p", "c_void_p", "c_void_p", "c_void_p"]


def test_python_refusals_need_no_device():
    from modulations_amd import crc
    from modulations_amd.dvb_rcs2_turbo import DVBRCS2_Turbo
    c = DVBRCS2_Turbo(48, "1/2", inv_perm="stable")
    assert crc.payload_bits(c, "crc16") == 80 and crc.payload_bits(c, "crc32") == 64
    with pytest.raises(ValueError):
        crc.payload_bits(c, "crc8")
    with pytest.raises(ValueError):
        crc.attach_device(None, "crc24")
    with pytest.raises(TypeError):
        crc.attach_device(np.zeros((2, 96), np.uint8), "crc16")


# ---- the BER tool's bookkeeping ------------------------------------------------------------

def test_ber_tool_keys_the_sweep_on_crc_and_ack_only_when_given():
    from modulations_amd import ber
    ap = ber.arg_parser()
    plain = ber.sweep_config(ap.parse_args(["--harq", "chase"]))
    assert "crc" not in plain and "ack" not in plain                      # existing result files still resume
    cfg = ber.sweep_config(ap.parse_args(["--harq", "chase", "--crc", "crc16"]))
    assert cfg == {**plain, "crc": "crc16"}
    cfg = ber.sweep_config(ap.parse_args(["--harq", "chase", "--crc", "crc32", "--ack", "crc"]))
    assert cfg == {**plain, "crc": "crc32", "ack": "crc"}
    assert "not charged" in " ".join(ap.format_help().split())            # the rate loss, said in the help


@pytest.mark.parametrize("argv", [["--ack", "crc", "--crc", "crc16"], ["--harq", "chase", "--ack", "crc"],
                                  ["--crc", "crc16", "--channel", "rayleigh", "--csi", "pilots"],
                                  ["--crc", "crc16", "--channel", "rayleigh", "--rx-branches", "2"], ["--crc", "crc8"]])
def test_ber_tool_refuses_what_the_frame_check_does_not_take(argv):
    from modulations_amd import ber
    with pytest.raises(SystemExit):
        ber.main(argv)
