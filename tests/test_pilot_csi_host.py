"""Pilot-aided channel estimation, host side: the ABI's names, the
layout's arithmetic, the Python refusals (all raised before any device call, so they are met
here with host tensors) and what the restated estimator (tests/pilot_csi_ref.py) recovers
from noise-free frames."""
import os
import re

import numpy as np
import pytest

import pilot_csi_ref as P
from modulations_amd import _native
from modulations_amd import demap as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tdec_csi_pilots_dev", "tdec_csi_strip_dev", "tdec_workload_frame_dev")


def test_new_names_are_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "tdec.h")).read()
    for name in NEW:
        assert name in _native.EXPORTS
        assert re.search(rf"^int {name}\(", src, re.M), name
        assert not name.startswith("tdec_demap")


@pytest.mark.parametrize("plen,dlen", [(1, 1), (2, 7), (4, 47), (5, 16)])
def test_layout_arithmetic(plen, dlen):
    lay = D.PilotLayout(plen, dlen)
    for J0 in (1, 3):
        for S in (1, dlen, J0 * dlen + 1):
            J = -(-S // dlen)
            assert lay.n_segments(S) == J == P.n_segments(S, dlen)
            assert lay.n_blocks(S) == J + 1
            T = S + (J + 1) * plen
            assert lay.frame_len(S) == T == P.frame_len(S, plen, dlen)
            Ls = [lay.segment_len(S, j) for j in range(J)]
            assert sum(Ls) == S and all(x == dlen for x in Ls[:-1]) and 1 <= Ls[-1] <= dlen
            assert Ls == [P.segment_len(S, dlen, j) for j in range(J)]
            # pilots and data tile the frame, in the order P0 D0 P1 ... D(J-1) PJ
            pos = np.concatenate([lay.pilot_positions(S), lay.data_positions(S)])
            assert sorted(pos.tolist()) == list(range(T))
            assert np.array_equal(lay.data_positions(S), P.data_positions(S, plen, dlen))
            for j in range(J):
                assert lay.block_start(S, j) + plen == lay.data_positions(S)[j * dlen]
                assert lay.data_positions(S)[j * dlen + Ls[j] - 1] + 1 == lay.block_start(S, j + 1)
            assert lay.block_start(S, J) + plen == T
            assert lay.block_start(S, J) == P.block_start(S, plen, dlen, J)
    assert D.PilotLayout(4, 18).n_blocks(72) == 5


def test_default_pilots_are_the_documented_formula():
    lay = D.PilotLayout(3, 5)
    p = lay.pilots(11)
    assert p.dtype == np.complex64 and len(p) == 4 * 3
    want = np.array([1j ** ((k * (k + 1) // 2) % 4) for k in range(12)])
    assert np.array_equal(p, want.astype(np.complex64))
    assert np.array_equal(p, P.default_pilots(12))
    assert np.all(np.abs(p) == 1) and len(set(p.tolist())) == 4
    assert np.array_equal(lay.pilots(11), lay.pilots(100)[:12])         # no RNG, no state


def test_layout_refusals():
    for plen, dlen in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            D.PilotLayout(plen, dlen)
    with pytest.raises(ValueError):
        D.PilotLayout(2, 4).frame_len(0)
    seq = np.ones(8, np.complex64)
    seq[4:6] = 0                                                        # block 2 of plen = 2
    with pytest.raises(ValueError, match="pilot block 2 has no energy"):
        D.PilotLayout(2, 3, sequence=seq).pilots(9)
    assert len(D.PilotLayout(2, 3, sequence=seq).pilots(3)) == 4        # S = 3 uses blocks 0 and 1 alone
    with pytest.raises(ValueError, match="needs 8"):
        D.PilotLayout(2, 3, sequence=seq[:6]).pilots(9)
    seq[4] = np.nan
    with pytest.raises(ValueError, match="no energy"):
        D.PilotLayout(2, 3, sequence=seq).pilots(9)


def test_python_refusals_come_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")

    def no_device_call():
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_native, "lib", no_device_call)
    lay = D.PilotLayout(2, 7)
    T = lay.frame_len(8)
    ok = torch.zeros((3, T), dtype=torch.complex64)
    for fn in (D.estimate_csi_device, D.strip_pilots_device):
        kw = {"noise_var": 0.1} if fn is D.estimate_csi_device else {}
        with pytest.raises(TypeError):                                   # dtype
            fn(ok.to(torch.complex128), lay, **kw)
        with pytest.raises(TypeError):
            fn(np.zeros((3, T), np.complex64), lay, **kw)
        with pytest.raises(TypeError):
            fn(ok, (2, 7), **kw)
        # shape: plen = 2, dlen = 7 frames are 5 .. 11 (S = 1 .. 7) or 14 .. 20 long, and so on
        for shape in ((T,), (3, T, 1), (0, T), (3, 2), (3, 4), (3, 12), (3, 13), (3, 22)):
            with pytest.raises(ValueError, match="frame length|2-D"):
                fn(torch.zeros(shape, dtype=torch.complex64), lay, **kw)
        with pytest.raises(ValueError, match="mode"):
            fn(ok, lay, mode="cubic", **kw)
        with pytest.raises(ValueError, match="HIP device"):             # device: a host tensor
            fn(ok, lay, **kw)
        seq = np.ones(6, np.complex64)
        seq[2:4] = 0
        with pytest.raises(ValueError, match="no energy"):              # zero-energy pilot block
            fn(ok, D.PilotLayout(2, 7, sequence=seq), **kw)
        with pytest.raises(ValueError, match="plen == 1"):              # nothing to estimate the noise from
            fn(torch.zeros((3, 3), dtype=torch.complex64), D.PilotLayout(1, 7),
               nv_rows_out=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="plen == 1"):                  # plen == 1 and no noise source
        D.estimate_csi_device(torch.zeros((3, 3), dtype=torch.complex64), D.PilotLayout(1, 7))
    with pytest.raises(ValueError, match="negative"):
        D.estimate_csi_device(ok, lay, noise_var=-0.5)
    with pytest.raises(TypeError):
        D.estimate_csi_device(ok, lay, noise_var=torch.zeros(3, dtype=torch.float32))
    with pytest.raises(ValueError, match="shape"):
        D.estimate_csi_device(ok, lay, noise_var=torch.zeros(4, dtype=torch.float64))


# ---- the restatement on noise-free frames -----------------------------------------------------
def _dyadic(rng, shape, bits=6):
    """Complex values whose parts are multiples of 2^-bits in [-2, 2]: sums and products of a
    few of them are exact in float64."""
    q = 2.0 ** -bits
    return (rng.integers(-2 / q, 2 / q + 1, shape) * q + 1j * rng.integers(-2 / q, 2 / q + 1, shape) * q)


def _frame(x, h_pos, pilots, S, plen, dlen):
    """Noise-free frames: position t carries h_pos[:, t] times its pilot or data symbol."""
    B = x.shape[0]
    T = P.frame_len(S, plen, dlen)
    tx = np.zeros((B, T), np.complex128)
    tx[:, P.data_positions(S, plen, dlen)] = x
    J = P.n_segments(S, dlen)
    for j in range(J + 1):
        t0 = P.block_start(S, plen, dlen, j)
        tx[:, t0:t0 + plen] = pilots[j * plen:(j + 1) * plen]
    return (h_pos * tx).astype(np.complex64)


@pytest.mark.parametrize("S,plen,dlen", [(1, 1, 1), (7, 2, 7), (8, 2, 7), (72, 5, 16), (289, 3, 47)])
def test_constant_gain_is_recovered_exactly(S, plen, dlen):
    rng = np.random.default_rng(S + plen)
    B = 5
    pilots = P.default_pilots((P.n_segments(S, dlen) + 1) * plen)
    x = _dyadic(rng, (B, S))
    h = _dyadic(rng, (B, 1), bits=4)
    h[h == 0] = 0.5 - 0.25j
    T = P.frame_len(S, plen, dlen)
    frames = _frame(x, np.broadcast_to(h, (B, T)), pilots, S, plen, dlen)
    for mode in ("linear", "mean"):
        r = P.estimate(frames, pilots, S, plen, dlen, mode=mode, nv=0.25)
        assert np.array_equal(r["hp"], np.broadcast_to(h, r["hp"].shape))
        assert np.array_equal(r["h"], np.broadcast_to(h, (B, S)).astype(np.complex64))
        assert np.array_equal(r["nv_sym"], np.broadcast_to(0.25 / (h.real * h.real + h.imag * h.imag), (B, S)))
        if plen >= 2:
            assert np.array_equal(r["nv"], np.full(B, 0.02))            # zero residual: the floor
    # a dyadic table point divided by a dyadic gain is not dyadic in general; with |h|^2 a power of two it is
    h2 = np.array([[1 + 1j], [2.0], [-0.5j], [0.25 - 0.25j], [-4 + 4j]])
    frames = _frame(x, np.broadcast_to(h2, (B, T)), pilots, S, plen, dlen)
    r = P.estimate(frames, pilots, S, plen, dlen, nv=1.0)
    assert np.array_equal(r["z"], x.astype(np.complex64))


@pytest.mark.parametrize("S,plen,dlen", [(7, 2, 7), (8, 2, 7), (72, 5, 16), (289, 3, 47), (48, 1, 16)])
def test_linear_gain_is_recovered_exactly_at_every_data_symbol(S, plen, dlen):
    """h(t) = h0 + t dh with dyadic h0, dh: a block's gain is h at the block's centre (the
    pilots have unit modulus: the weights are equal), and the interpolation weight is the
    symbol's position between two centres.  The last segment may be short: its weight's
    denominator is then 2 (plen + L) with the short L, and the centres still bracket it."""
    rng = np.random.default_rng(S * plen)
    B = 4
    pilots = P.default_pilots((P.n_segments(S, dlen) + 1) * plen)
    T = P.frame_len(S, plen, dlen)
    h0 = _dyadic(rng, (B, 1), bits=3)
    dh = _dyadic(rng, (B, 1), bits=3) * 2.0 ** -9
    t = np.arange(T)[None, :]
    h_pos = h0 + t * dh
    frames = _frame(np.ones((B, S)), h_pos, pilots, S, plen, dlen)
    assert np.array_equal(frames.astype(np.complex128)[:, P.data_positions(S, plen, dlen)],
                          h_pos[:, P.data_positions(S, plen, dlen)])     # the frames themselves are exact
    r = P.estimate(frames, pilots, S, plen, dlen, nv=0.1)
    want = h_pos[:, P.data_positions(S, plen, dlen)]
    # the weights' denominators 2 (plen + L) are not powers of two: the product w (b - a) rounds
    # once in float64, far below float32's resolution, so the float32 gains are exact
    assert np.array_equal(r["h"], want.astype(np.complex64))
    centres = np.array([P.block_start(S, plen, dlen, j) + (plen - 1) / 2 for j in range(r["hp"].shape[1])])
    assert np.array_equal(r["hp"], h0 + centres[None, :] * dh)


def test_rotation_is_tracked_to_the_chord_bound():
    """A unit gain rotating by f = 1e-4 cycles per symbol: the interpolated gain is within
    theta^2 / 8 * 1.5 of the true one, theta = 2 pi f (plen + dlen) the angle between two
    block centres and theta^2 / 8 the chord-to-arc distance of linear interpolation on the
    unit circle (the block gain itself is the mean of plen points of the arc, inside the
    circle by less than that again: hence the factor)."""
    S, plen, dlen, f = 4 * 47 + 11, 4, 47, 1e-4
    pilots = P.default_pilots((P.n_segments(S, dlen) + 1) * plen)
    T = P.frame_len(S, plen, dlen)
    t = np.arange(T)
    rng = np.random.default_rng(5)
    rot = np.exp(2j * np.pi * f * t)[None, :]
    frames = _frame(np.exp(2j * np.pi * rng.random((1, S))), rot, pilots, S, plen, dlen)
    r = P.estimate(frames, pilots, S, plen, dlen, nv=0.1)
    theta = 2 * np.pi * f * (plen + dlen)
    err = np.abs(r["h"].astype(np.complex128) - rot[:, P.data_positions(S, plen, dlen)])
    print("max |h - true|", err.max(), "bound", theta ** 2 / 8 * 1.5)
    assert err.max() <= theta ** 2 / 8 * 1.5


def test_zero_and_nonfinite_blocks_erase_their_segments_in_the_restatement():
    S, plen, dlen = 20, 2, 5
    pilots = P.default_pilots(5 * plen)
    rng = np.random.default_rng(9)
    x = _dyadic(rng, (3, S))
    frames = _frame(x, np.ones((3, P.frame_len(S, plen, dlen))), pilots, S, plen, dlen)
    frames[0, P.block_start(S, plen, dlen, 2)] = np.nan                 # block 2: segments 1 and 2
    frames[1, P.block_start(S, plen, dlen, 0):P.block_start(S, plen, dlen, 0) + plen] = 0   # block 0: segment 0
    frames[2, P.block_start(S, plen, dlen, 4) + 1] = np.inf             # block 4: segment 3
    for mode in ("linear", "mean"):
        r = P.estimate(frames, pilots, S, plen, dlen, mode=mode, nv=0.1)
        erased = np.isposinf(r["nv_sym"]) & (r["z"] == 0)
        want = np.zeros((3, S), bool)
        want[0, 5:15] = want[1, 0:5] = want[2, 15:20] = True
        assert np.array_equal(erased, want)
        assert np.array_equal(r["z"][~want], x.astype(np.complex64)[~want])


def test_ber_records_the_pilot_options_only_when_used():
    from modulations_amd import ber
    ap = ber.arg_parser()
    base = ["--channel", "rayleigh", "--coherence", "424"]
    known = ber.sweep_config(ap.parse_args(base))
    assert not {"csi", "pilot_len", "pilot_spacing", "cfo", "csi_noise"} & set(known)
    assert known == ber.sweep_config(ap.parse_args(base + ["--csi", "known", "--pilot-len", "9", "--cfo", "1e-3"]))
    pil = ber.sweep_config(ap.parse_args(base + ["--csi", "pilots", "--pilot-spacing", "53", "--cfo", "1e-4"]))
    assert {k: pil[k] for k in set(pil) - set(known)} == {"csi": "pilots", "pilot_len": 4, "pilot_spacing": 53,
                                                         "cfo": 1e-4, "csi_noise": "known"}
    assert "csi" not in ber.sweep_config(ap.parse_args([]))                # awgn: as before
