"""References and pattern builders for the burst detector's run search and its
smoothing (mdm_burst_find: k_bf_smooth, k_bf_flags, k_bf_scan).  numpy only:
no GPU, no torch.

  first_run      the reference's search (sdr_modem.py:538-542) as a sliding count
  literal_first_run  the same, as the reference's own loop (slow; the host test
                 pins first_run to it)
  scan_model     the three-level search as the kernels do it (per-tile first /
                 last / start, 256-tile chunks with a carried last zero), with
                 the set of branches the input takes
  flags_to_signal  a capture whose device flags are exactly the designed ones
  DESIGNED       patterns aimed at one path each (designed())
  random_flags   alternating runs around the lengths half - 1, half, half + 1
  smooth_ref     np.convolve(power, ones(win) / win, 'same') in long double

TEST INFRASTRUCTURE ONLY."""
import numpy as np

TILE = 1024      # BF_TILE: positions per workgroup of k_bf_flags
CHUNK = 256      # tiles per pass of k_bf_scan's loop
BIG_N = 513 * TILE + 7      # three passes of the chunk loop (514 tiles)

BRANCHES = ("cross_tile_run", "run_from_index_0", "tile_local_start", "tile_without_zero", "second_chunk",
            "carry_used", "tail_run", "limit_rejects")


def first_run(flags, pre):
    """First i < n - pre with flags[i : i + pre // 2] all set, else -1 (a sliding count)."""
    half = pre // 2
    c = np.concatenate([[0], np.cumsum(flags.astype(np.int64))])
    ok = (c[half:] - c[:max(len(c) - half, 0)]) == half  # ok[i]: flags[i:i+half] all set
    idx = np.nonzero(ok[:max(len(flags) - pre, 0)])[0]
    return int(idx[0]) if len(idx) else -1


def literal_first_run(flags, pre):
    """sdr_modem.py:538-542 as written there."""
    f = np.asarray(flags, bool)
    for i in range(len(f) - pre):
        if f[i:i + pre // 2].all():
            return i
    return -1


def scan_model(flags, pre):
    """(answer, branches) of the search as k_bf_flags and k_bf_scan run it.

    Per tile of 1024 positions (positions past n count as set): first = the first zero flag,
    last = the last one, start = the first p + 1 behind a zero p whose next zero in the tile is
    >= half away (all tile-local, -1 = none).  Then one pass per 256 tiles: every tile gets the
    last zero before it (a prefix maximum inside the pass, the carry from the passes before);
    a tile with a zero proposes prev + 1 if its first zero is >= half behind prev, else its own
    start; the smallest proposal of a pass ends the search.  Without any, the run behind the
    last zero reaches the end.  The answer must lie below n - pre."""
    f = np.asarray(flags, bool)
    n, half = len(f), pre // 2
    n_tiles = -(-n // TILE)
    first = np.full(n_tiles, -1, np.int64)
    last = np.full(n_tiles, -1, np.int64)
    start = np.full(n_tiles, -1, np.int64)
    for g in range(n_tiles):
        zs = np.nonzero(~f[g * TILE:(g + 1) * TILE])[0]
        if len(zs):
            first[g], last[g] = zs[0], zs[-1]
            wide = np.nonzero(zs[1:] - zs[:-1] - 1 >= half)[0]
            if len(wide):
                start[g] = zs[wide[0]] + 1
    taken = set()
    carry, found, passes, win_tile = -1, -1, 0, n_tiles
    for c0 in range(0, n_tiles, CHUNK):
        passes += 1
        best, best_kind, running = None, None, -1
        for g in range(c0, min(c0 + CHUNK, n_tiles)):
            base = g * TILE
            prev = max(carry, running)
            if first[g] >= 0:
                cand = kind = None
                if base + first[g] - prev - 1 >= half:
                    cand = prev + 1
                    kind = {"run_from_index_0" if prev < 0 else "cross_tile_run"}
                    if carry > running and carry >= 0:
                        kind.add("carry_used")
                elif start[g] >= 0:
                    cand, kind = base + start[g], {"tile_local_start"}
                if cand is not None and (best is None or cand < best):
                    best, best_kind, win_tile = cand, kind, g
                running = max(running, base + last[g])
        if best is not None:
            found = best
            taken |= best_kind
            break
        carry = max(carry, running)
    if passes > 1:
        taken.add("second_chunk")
    if found < 0:
        found = carry + 1
        taken.add("tail_run")
        if carry >= 0 and passes > 1 and carry < (passes - 1) * CHUNK * TILE:
            taken.add("carry_used")
    # a tile without a zero between the run's start and the tile that closed it (or the end)
    lo = max(found, 0) // TILE
    if np.any(first[lo:min(win_tile + 1, n_tiles)] < 0):
        taken.add("tile_without_zero")
    if not found < n - pre:
        taken.add("limit_rejects")
        found = -1
    return int(found), taken


def flags_to_signal(flags, dtype):
    """Amplitude 1.0 where the flag is set, 0.5 where clear, imaginary part 0.  With win = 1
    the prefix sums add 1.0 and 0.25 (exact), so smooth == power bit for bit, max == 1, the
    threshold is 0.3 and the device's flags are the designed ones (given one flag is set)."""
    f = np.asarray(flags, bool)
    x = np.where(f, 1.0, 0.5).astype(dtype)
    assert x.dtype in (np.complex64, np.complex128)
    p = np.abs(x) ** 2
    assert np.all((p == 1.0) | (p == 0.25)) and np.array_equal(p == 1.0, f)
    return x


# ---------------------------------------------------------------- designed patterns ------------
def _runs(n, *runs):
    """All clear, but for the set runs [a, b)."""
    f = np.zeros(n, bool)
    for a, b in runs:
        assert 0 <= a < b <= n, (a, b, n)
        f[a:b] = True
    return f


def run_from_index_0(n, pre, short=False):
    """A run from index 0 of half (half - 1) flags, a qualifying run inside tile 1 later."""
    half = pre // 2
    return _runs(n, (0, half - short), (2000, 2000 + half))


def gap_in_tile(n, pre, first_set, short=False, later=True):
    """Two zeros of tile 1 with half (half - 1) set flags between them, the first set flag at
    tile-local position first_set; a qualifying run in tile 3 behind it."""
    half = pre // 2
    a = TILE + first_set
    runs = [(a, a + half - short)]
    if later:
        runs.append((3 * TILE + 17, 3 * TILE + 17 + half))
    return _runs(n, *runs)


def cross_tile(n, pre, short=False):
    """A run of half (half - 1) flags over the boundary of tiles 0 and 1; a qualifying run in tile 2."""
    half = pre // 2
    a = TILE - half // 2
    return _runs(n, (a, a + half - short), (2 * TILE + 100, 2 * TILE + 100 + half))


def full_tiles_inside(n, pre, short=False):
    """half > 2048: tiles 1 and 2 lie inside the run, without a zero."""
    half = pre // 2
    assert half > 2 * TILE
    return _runs(n, (1000, 1000 + half - short))


def reaches_end(n, pre, accepted, zero_at_end):
    """A run from n - pre - 1 (accepted) or n - pre (rejected) to the last sample, or to the one
    before it with the last zero at n - 1."""
    return _runs(n, (n - pre - (1 if accepted else 0), n - (1 if zero_at_end else 0)))


def decoys(n, pre):
    """Five runs of half - 1, two of them over a tile boundary, before the first qualifying one."""
    half = pre // 2
    d = half - 1
    return _runs(n, (500, 500 + d), (TILE - 10, TILE - 10 + d), (1500, 1500 + d), (2 * TILE - 5, 2 * TILE - 5 + d),
                 (2600, 2600 + d), (3 * TILE - 12, 3 * TILE - 12 + half))


def chunk_boundary_cross(n, pre, tile=512):
    """The only qualifying run starts in tile `tile` - 1 and ends in `tile`, the first of a chunk."""
    half = pre // 2
    a = tile * TILE - half // 3 - 1
    return _runs(n, (a, a + half))


def chunk_boundary_start(n, pre, tile=512):
    """The run starts at position 0 of the chunk's first tile, behind a zero at position 1023."""
    return _runs(n, (tile * TILE, tile * TILE + pre // 2))


def set_from_tile(n, pre, tile=300):
    """All flags set from tile `tile` to the end: found = carry + 1 after every pass."""
    return _runs(n, (tile * TILE, n))


def zeros_only_at_head(n, pre, head=5000):
    """Clear up to `head`, set from there on: whole chunks of tiles without a zero."""
    return _runs(n, (head, n))


def all_set(n, pre):
    return np.ones(n, bool)


def none_set(n, pre):
    return np.zeros(n, bool)


def single_flag(n, pre, at):
    return _runs(n, (at, at + 1))


class Pattern:
    def __init__(self, name, n, pre, flags, branch):
        assert len(flags) == n and flags.dtype == bool
        self.name, self.n, self.pre, self.flags, self.branch = name, n, pre, flags, branch

    def __repr__(self):
        return self.name


def designed():
    """Every designed pattern, with the branch of scan_model it is named after."""
    P = []

    def add(name, n, pre, flags, branch):
        P.append(Pattern(f"{name}-n{n}-pre{pre}", n, pre, flags, branch))

    for pre in (64, 65):
        add("run_from_index_0", 4097, pre, run_from_index_0(4097, pre), "run_from_index_0")
        add("run_from_index_0_short", 4097, pre, run_from_index_0(4097, pre, short=True), "tile_local_start")
        add("cross_tile", 4096, pre, cross_tile(4096, pre), "cross_tile_run")
        add("cross_tile_short", 4096, pre, cross_tile(4096, pre, short=True), "tile_local_start")
    # half = 3: the run 4k+2 .. 4k+4 (short: 4k+3, 4k+4) over a thread boundary, 254 .. 256 (255, 256)
    # over a wave boundary, and 1020 .. 1022 (1021, 1022) with the closing zero at position 1023
    for pre in (6, 7):
        for where, at in (("thread", 4 * 37 + 2), ("wave", 254), ("tile_end", 1020)):
            add(f"gap_{where}", 5000, pre, gap_in_tile(5000, pre, at), "tile_local_start")
            add(f"gap_{where}_short", 5000, pre, gap_in_tile(5000, pre, at + 1, short=True), "tile_local_start")
            add(f"gap_{where}_short_alone", 5000, pre, gap_in_tile(5000, pre, at + 1, short=True, later=False),
                None)
    # a wider gap inside one tile, from a wave's last position to far into the next wave
    add("gap_wave_wide", 3000, 140, gap_in_tile(3000, 140, 255, later=False), "tile_local_start")
    add("full_tiles_inside", 10 * TILE + 3, 5000, full_tiles_inside(10 * TILE + 3, 5000), "tile_without_zero")
    add("full_tiles_inside_short", 10 * TILE + 3, 5000, full_tiles_inside(10 * TILE + 3, 5000, short=True), None)
    for n in (3 * TILE, 3 * TILE + 1):
        for pre in (700, 1500):
            add("reaches_end_accepted", n, pre, reaches_end(n, pre, True, False), "tail_run")
            add("reaches_end_rejected", n, pre, reaches_end(n, pre, False, False), "limit_rejects")
            # the closing zero n - 1 is the run's own tile's only for pre = 700, n = 3 tiles
            add("zero_at_end_accepted", n, pre, reaches_end(n, pre, True, True),
                "tile_local_start" if (pre, n) == (700, 3 * TILE) else "cross_tile_run")
            add("zero_at_end_rejected", n, pre, reaches_end(n, pre, False, True), "limit_rejects")
    add("decoys", 8192, 64, decoys(8192, 64), "cross_tile_run")
    for pre in (64, 701):
        add("chunk_boundary_cross_512", BIG_N, pre, chunk_boundary_cross(BIG_N, pre), "carry_used")
        add("chunk_boundary_cross_256", BIG_N, pre, chunk_boundary_cross(BIG_N, pre, 256), "carry_used")
        add("chunk_boundary_start_512", BIG_N, pre, chunk_boundary_start(BIG_N, pre), "carry_used")
        add("set_from_tile_300", BIG_N, pre, set_from_tile(BIG_N, pre), "tail_run")
        add("zeros_only_at_head", BIG_N, pre, zeros_only_at_head(BIG_N, pre), "tile_without_zero")
    add("set_from_tile_513", BIG_N, 4, set_from_tile(BIG_N, 4, 513), "tail_run")
    add("set_from_tile_513_rejected", BIG_N, 8, set_from_tile(BIG_N, 8, 513), "limit_rejects")
    add("all_set", 3000, 64, all_set(3000, 64), "tail_run")
    add("all_set_one_tile", TILE, 64, all_set(TILE, 64), "tail_run")
    add("none_set", 3000, 64, none_set(3000, 64), "limit_rejects")
    add("n_equals_pre", 1500, 1500, all_set(1500, 1500), "limit_rejects")
    add("n_below_pre", 1500, 2000, all_set(1500, 2000), "limit_rejects")
    add("single_sample", 1, 0, all_set(1, 0), "tail_run")
    for pre in (0, 1):
        add("none_set", 2500, pre, none_set(2500, pre), "run_from_index_0")
        add("all_set", 2500, pre, all_set(2500, pre), "tail_run")
        add("first_tile_set", 2500, pre, _runs(2500, (0, TILE)), "run_from_index_0")
    for at in (0, 5, 1023, 1024, 2047):
        add(f"single_flag_at_{at}", 2 * TILE + 4, 3, single_flag(2 * TILE + 4, 3, at), None)
    add("single_flag_accepted", 2 * TILE, 3, single_flag(2 * TILE, 3, 2 * TILE - 4), "tile_local_start")
    add("single_flag_rejected", 2 * TILE, 3, single_flag(2 * TILE, 3, 2 * TILE - 3), "limit_rejects")
    names = [p.name for p in P]
    assert len(set(names)) == len(names)
    return P


def random_flags(rng, n, half):
    """Alternating set and clear runs.  Set runs: 1, 2, half - 1, half, half + 1 or uniform in
    [1, 3 half + 1]; clear runs: 1, 1, 2 or uniform in [1, half + 1]."""
    m = n // 2 + 1                       # runs of each kind: every run has >= 1 flag
    s = np.stack([np.full(m, 1), np.full(m, 2), np.full(m, half - 1), np.full(m, half), np.full(m, half + 1),
                  rng.integers(1, 3 * half + 2, m)])[rng.integers(0, 6, m), np.arange(m)]
    c = np.stack([np.full(m, 1), np.full(m, 1), np.full(m, 2),
                  rng.integers(1, half + 2, m)])[rng.integers(0, 4, m), np.arange(m)]
    lens = np.empty(2 * m, np.int64)
    first_set = bool(rng.integers(0, 2))
    lens[0::2], lens[1::2] = (s, c) if first_set else (c, s)
    lens = np.maximum(lens, 1)
    vals = np.zeros(2 * m, bool)
    vals[0::2], vals[1::2] = first_set, not first_set
    k = int(np.searchsorted(np.cumsum(lens), n)) + 1
    return np.repeat(vals[:k], lens[:k])[:n]


# ---------------------------------------------------------------- smoothing --------------------
def smooth_ref(p, win):
    """np.convolve(p, ones(win) / win, 'same') for len(p) >= win, in long double:
    smooth[i] = sum(p[i - win // 2 : i - win // 2 + win]) / win, zero outside [0, n)."""
    n = len(p)
    assert n >= win >= 1
    c = np.concatenate([[0], np.cumsum(np.asarray(p).astype(np.longdouble))])
    lo = np.arange(n) - win // 2
    return (c[np.clip(lo + win, 0, n)] - c[np.clip(lo, 0, n)]) / np.longdouble(win)
