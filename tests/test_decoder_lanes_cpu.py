"""The lane layout of the two-team decoder (sh_decoder_lanes, sh_sched.h) on the host, through scrappie_hip_decoder_lanes.

The layout lays a launch group's tiles end to end over one lane per workgroup and cuts only where a lane is full.  k_ff_viterbi_teams steps
two blocks at a time, so the rule counts in block PAIRS: a tile of T blocks costs ceil(T / 2) pair steps, M / 2 = max(longest tile's pairs,
ceil(sum of pairs / lanes)), and a cut falls between two pairs.  What the kernel relies on, checked here:
  * every block of every live tile is covered exactly once, dead tiles never;
  * every cut is even (only a tile's true end may be odd);
  * no lane is longer than M (in blocks, and in pair steps: the time it really takes);
  * a cut tile has two segments, ordinals 0 and 1; the producing one (ordinal 0) opens a lane in a LOWER-numbered workgroup, the consuming
    one closes its lane, and the producer's last pair step comes no later than the consumer's first (index <=): the consumer's wait on the
    arrival flag never depends on a workgroup that itself waits;
  * with no more live tiles than CUs the tiles stay whole, one per workgroup;
  * ordinals count up within a tile in block order."""
import ctypes as C

import numpy as np
import pytest

import scrappie_amd as sa

ip = C.POINTER(C.c_int)


def _lanes(tile_T, ncu):
    L = sa.lib()
    L.scrappie_hip_decoder_lanes.restype = C.c_long
    L.scrappie_hip_decoder_lanes.argtypes = [ip, C.c_size_t, C.c_int, ip, ip, ip, ip, C.c_size_t]
    tt = np.ascontiguousarray(tile_T, dtype=np.int32)
    cap = len(tt) + ncu + 4
    lane_off = np.full(ncu + 1, -1, np.int32)
    seg = np.zeros((cap, 4), np.int32)
    nwg, M = C.c_int(), C.c_int()
    ns = L.scrappie_hip_decoder_lanes(tt.ctypes.data_as(ip), len(tt), ncu, C.byref(nwg), C.byref(M), lane_off.ctypes.data_as(ip),
                                      seg.ctypes.data_as(ip), cap)
    assert 0 <= ns <= cap
    return nwg.value, M.value, lane_off[:nwg.value + 1].copy(), seg[:ns].copy()


def _check(tile_T, ncu):
    tt = np.asarray(tile_T, dtype=np.int64)
    nwg, M, lane_off, seg = _lanes(tt, ncu)
    live = [i for i, t in enumerate(tt) if t > 0]
    assert nwg == min(ncu, len(live))                          # the grid: min(CUs, live tiles)
    if not live:
        assert len(seg) == 0
        return nwg, M, lane_off, seg
    assert lane_off[0] == 0 and lane_off[-1] == len(seg) and np.all(np.diff(lane_off) >= 0)      # (the lowest workgroups may stay empty: nine one-pair tiles on four lanes of three)
    pairs = (tt + 1) // 2
    assert M % 2 == 0 and M == 2 * max(int(pairs.max()), -(-int(pairs.sum()) // nwg))
    covered = {t: np.zeros(int(tt[t]), np.int32) for t in live}
    by_tile = {}
    for wg in range(nwg):
        rows = seg[lane_off[wg]:lane_off[wg + 1]]
        blocks = steps = 0
        for k, (tile, s0, s1, ordinal) in enumerate(rows):
            tile, s0, s1 = int(tile), int(s0), int(s1)
            assert tile in covered and 0 <= s0 < s1 <= tt[tile]
            assert s0 % 2 == 0 and (s1 % 2 == 0 or s1 == tt[tile])         # even cuts
            covered[tile][s0:s1] += 1
            by_tile.setdefault(tile, []).append(dict(wg=wg, s0=s0, s1=s1, ord=int(ordinal), start=steps, end=steps + (s1 - s0 + 1) // 2,
                                                     first=(k == 0), last=(k == len(rows) - 1)))
            blocks += s1 - s0
            steps += (s1 - s0 + 1) // 2
        assert blocks <= M and 2 * steps <= M                               # lane capacity
    assert all(np.all(c == 1) for c in covered.values())                    # every block exactly once
    ncut = 0
    for tile, ps in by_tile.items():
        ps.sort(key=lambda p: p["s0"])
        assert [p["ord"] for p in ps] == list(range(len(ps))) and len(ps) <= 2      # ordinals count up; M >= the longest tile: one cut at most
        if len(ps) == 2:
            ncut += 1
            head, tail = ps
            assert head["s1"] == tail["s0"]
            assert head["wg"] < tail["wg"]                                  # the producer in the lower-numbered workgroup
            assert head["first"] and tail["last"]                           # it opens its lane (never waits); the consumer closes its own
            assert head["end"] <= tail["start"]                             # and is through before the consumer starts
    assert ncut <= nwg - 1
    if len(live) <= ncu:
        assert ncut == 0 and len(seg) == len(live) and np.all(np.diff(lane_off) == 1)      # whole tiles, as K = 1 was
    return nwg, M, lane_off, seg


HAND = {
    "equal": ([800] * 625, 256),
    "equal-odd": ([37] * 11, 4),
    "one-long": ([400] + [20] * 30, 8),
    "one-long-odd": ([401] + [21] * 30, 8),
    "odd-lengths": ([2 * i + 1 for i in range(40, 0, -1)], 7),
    "one-block-tiles": ([1] * 9, 2),
    "dead-tiles": ([50, 44, 0, 31, 0, 17, 3, 0, 0], 3),
    "all-dead": ([0, 0, 0], 4),
    "fewer-than-cus": ([60, 33, 33, 2], 8),
    "as-many-as-cus": ([9, 8, 7, 6], 4),
    "one-more-than-cus": ([9, 8, 7, 6, 5], 4),
    "one-cu": ([13, 12, 11], 1),
    "five-on-two": ([27] * 5, 2),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_layouts(name):
    tt, ncu = HAND[name]
    _check(tt, ncu)


@pytest.mark.parametrize("seed", range(12))
def test_random_layouts(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 700))
    ncu = int(rng.choice([1, 2, 3, 8, 64, 256]))
    tt = np.sort(rng.integers(1, int(rng.choice([4, 60, 900])), n))[::-1].copy()      # the engine sorts tiles by length
    if seed % 3 == 0:
        tt[rng.integers(0, n, max(n // 10, 1))] = 0
    if seed % 4 == 1:
        tt = rng.permutation(tt)                                                       # the rule does not need the order
    _check(tt, ncu)


def test_the_flagship_group():
    """625 tiles of 800 blocks on 256 CUs: M = 1954 blocks against five equal pieces of 400 = 2000; 255 cuts against 625"""
    nwg, M, lane_off, seg = _check([800] * 625, 256)
    assert nwg == 256 and M == 1954 and len(seg) == 625 + 255
    assert int(np.max(np.diff(lane_off))) <= 4
