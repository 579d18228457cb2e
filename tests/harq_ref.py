"""Numpy restatement of hybrid ARQ soft combining.

TEST INFRASTRUCTURE (a plain module like fading_ref.py: numpy only, no GPU, nothing
imported from the package under test).  Restated here, from the issue's contract and
the reference's de-puncture loop (dvb_rcs2_turbo.py:476-487), not from the library:

  redundancy_version(punct, rv)   every parity row shifted cyclically by rv phases
  walk(n, punct)                  src[6][n]: the LLR index each plane component of a step
                                  takes (-1: not transmitted), and the walk's length
  accumulate(planes6, llr, ...)   planes6 [B][N][6] float32 {A, B, W1, Y1, W2, Y2} +=
                                  the de-punctured rows, one float32 add per transmitted
                                  component in call order, the others left untouched
  to_tiles / from_tiles           [B][N][6] <-> the decoder's tile layout (include/harq.h)
  llr6(planes6)                   the rate-1/3 LLR vector [B][6N] a decoder of the mother
                                  code reads from those planes
"""
import numpy as np

ROWS = ("W1", "Y1", "W2", "Y2")
TILE = 64


def redundancy_version(punct, rv):
    per = punct["period"]
    assert 0 <= rv < per
    out = {"period": per}
    for key in ROWS:
        out[key] = [punct[key][(p + rv) % per] for p in range(per)]
    return out


def walk(n, punct):
    """(src int64 [6][n], length): :476-487, A and B of every couple, then the parities
    the pattern transmits at phase i % period, in the order W1, Y1, W2, Y2."""
    src = np.full((6, n), -1, np.int64)
    idx = 0
    for i in range(n):
        p = i % punct["period"]
        src[0, i], src[1, i] = idx, idx + 1
        idx += 2
        for r, key in enumerate(ROWS):
            if punct[key][p]:
                src[2 + r, i] = idx
                idx += 1
    return src, idx


def transmitted(punct):
    """{(row, phase)} the pattern sends, rows named W1, Y1, W2, Y2."""
    return {(key, p) for key in ROWS for p in range(punct["period"]) if punct[key][p]}


def accumulate(planes6, llr, n, punct, row_of=None):
    """In place: slot c of planes6 [B][n][6] takes row row_of[c] of llr (None: row c); an
    entry outside [0, rows) leaves the slot untouched.  llr of any float dtype is rounded
    to float32 first (:466), then one float32 add per transmitted component."""
    assert planes6.dtype == np.float32 and planes6.shape[1:] == (n, 6)
    llr = np.asarray(llr)
    src, length = walk(n, punct)
    assert llr.shape[1] >= length
    B = planes6.shape[0]
    rows = np.arange(B) if row_of is None else np.asarray(row_of, np.int64)
    assert rows.shape == (B,)
    if row_of is None:
        assert llr.shape[0] == B
    sel = np.nonzero((rows >= 0) & (rows < llr.shape[0]))[0]
    with np.errstate(invalid="ignore", over="ignore"):
        l32 = llr[rows[sel]].astype(np.float32)
        for comp in range(6):
            k = np.nonzero(src[comp] >= 0)[0]
            at = (sel[:, None], k[None, :], comp)
            planes6[at] = planes6[at] + l32[:, src[comp][k]]
    return planes6


def tile_floats(n):
    return n * TILE * 6


def to_tiles(planes6, fill=0.0):
    """The tile layout as a flat float32 array of ceil(B / 64) tiles: per tile [n][64]
    float4 {A, B, W1, Y1}, then [n][64] float2 {W2, Y2}.  Idle lanes of the last tile: fill."""
    B, n, _ = planes6.shape
    tiles = -(-B // TILE)
    pad = np.full((tiles * TILE, n, 6), fill, np.float32)
    pad[:B] = planes6
    pad = pad.reshape(tiles, TILE, n, 6).transpose(0, 2, 1, 3)          # [tile][k][lane][6]
    out = np.empty((tiles, tile_floats(n)), np.float32)
    out[:, :n * TILE * 4] = pad[..., :4].reshape(tiles, -1)
    out[:, n * TILE * 4:] = pad[..., 4:].reshape(tiles, -1)
    return out.reshape(-1)


def from_tiles(flat, B, n):
    """[B][n][6] float32 read back from the tile layout."""
    tiles = -(-B // TILE)
    flat = np.asarray(flat, np.float32)[:tiles * tile_floats(n)].reshape(tiles, tile_floats(n))
    x = flat[:, :n * TILE * 4].reshape(tiles, n, TILE, 4)
    z = flat[:, n * TILE * 4:].reshape(tiles, n, TILE, 2)
    return np.concatenate([x, z], axis=3).transpose(0, 2, 1, 3).reshape(tiles * TILE, n, 6)[:B].copy()


def llr6(planes6):
    """The rate-1/3 walk of the planes: A, B, W1, Y1, W2, Y2 of every couple in turn."""
    return np.ascontiguousarray(planes6.reshape(planes6.shape[0], -1))


def same_bits(a, b):
    """Bit for bit where neither is NaN, and NaN at the same positions."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
