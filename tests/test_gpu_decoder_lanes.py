"""The two-team decoder walking a lane of segments, byte for byte, on small launch groups (run with -m gpu on an MI355X).

k_ff_viterbi_teams no longer owns one piece of a tile per workgroup: its workgroups walk the lane layout of sh_decoder_lanes (sh_sched.h) --
tiles end to end, cut only where a lane is full, on even blocks -- and run per SEGMENT what they ran once: the S1 team's prologue, the score
load (initial state or hand-over buffer), the wait on the arrival flag, the hand-over or final-state epilogue, producer 3's parked values.
A real layout needs more tiles than CUs (thousands of reads); the debug option "decoder_lanes" makes the layout for a device of that many
CUs, so with 2 a group of three or five tiles runs on two workgroups.  The construction is test_gpu_decoder_bytes.py's (logit table, one-hot
trunk activations, pinned tie columns); every case decodes one group with the teams kernel on lanes, with k_ff_lds + k_viterbi
("ff_separate") and with k_ff_viterbi ("fv_single") -- those two cut into two equal pieces a tile ("decoder_cus" = 2), through their own
hand-over -- and asks for identical traceback bytes of live states, end-state pointers, final states and scores, the final scores of every
state including the start / end slots, and the calls (the homopolymer pass reads hp_side).

Shapes (lanes = 2; the layouts are asserted below from the planner, so a change of the rule shows here first):
  odd       80 reads of 21 blocks (five tiles of 11 pairs, M = 56): workgroup 1 runs tile 0, tile 1 and blocks 10 .. 20 of tile 2 (a take-over
            behind two whole tiles, an odd end), workgroup 0 opens with blocks 0 .. 9 of tile 2 (a lane that starts with a cut tile and hands it
            over first thing) and goes on with two whole tiles: three segments each;
  ragged    16 reads of 60 blocks, 16 of 21, 23 .. 51, 48 of 20 (M = 86): workgroup 0 walks FOUR segments; the cut tile is the ragged one, cut
            at block 26 -- the reads of 21, 23 and 25 blocks end before the cut and their scores, start and end state cross the hand-over unchanged;
  one-block 16 reads of 41 blocks, 16 of 23, and a tile of 21 whose other reads have 3 .. 9 blocks (one-tap model; M = 44): tile 1 is cut at
            block 22 and its second segment is ONE block -- a pair of which the second block is skipped, behind a take-over.
A read of one block cannot be fed to any decoder form (the engine's min_samples: three blocks for the one-tap model, twelve for the shipped
window, see test_gpu_decoder_bytes.py); the shortest reads here are the three-block ones, and the one-block case is the one-block segment."""
import ctypes as C

import numpy as np
import pytest

import scrappie_amd as sa
from test_gpu_decoder_bytes import _same, _tb_state, eng, tables  # noqa: F401  (fixtures)
from test_gpu_decoder_pieces import _group

pytestmark = pytest.mark.gpu

LANES = 2
_TURN80 = [i % 4 for i in range(80)]
_TURN48 = [i % 4 for i in range(48)]
SHAPES = {
    "odd": ("tab5", [21] * 80, _TURN80),
    "ragged": ("tab5", [60] * 16 + list(range(21, 52, 2)) + [20] * 48, _TURN80),
    "one-block": ("tab1", [41] * 16 + [23] * 16 + [21] + [3, 4, 5, 6, 7, 8, 9] * 2 + [3], _TURN48),
}
# what the planner must give for each shape: segments per workgroup, the cut (tile, block)
LAYOUT = {"odd": ([3, 3], (2, 10)), "ragged": ([4, 2], (1, 26)), "one-block": ([2, 2], (1, 22))}
KWS = [dict(), dict(local_pen=150.0, skip_pen=0.25)]


def _plan(blocks):
    ip = C.POINTER(C.c_int)
    L = sa.lib()
    L.scrappie_hip_decoder_lanes.restype = C.c_long
    L.scrappie_hip_decoder_lanes.argtypes = [ip, C.c_size_t, C.c_int, ip, ip, ip, ip, C.c_size_t]
    srt = np.sort(np.asarray(blocks))[::-1]
    tt = np.ascontiguousarray([srt[i:i + 16].max() for i in range(0, len(srt), 16)], dtype=np.int32)
    lane_off = np.zeros(LANES + 1, np.int32)
    seg = np.zeros((len(tt) + LANES + 4, 4), np.int32)
    nwg = C.c_int()
    ns = L.scrappie_hip_decoder_lanes(tt.ctypes.data_as(ip), len(tt), LANES, C.byref(nwg), None, lane_off.ctypes.data_as(ip),
                                      seg.ctypes.data_as(ip), len(seg))
    return nwg.value, lane_off, seg[:ns], tt


def _reset(eng):
    for k in ("ff_separate", "fv_single", "dump_final", "decoder_cus", "decoder_lanes"):
        eng.debug_option(k, 0)
    eng.set_trunk_input(None)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_layouts_are_what_the_cases_are_about(name):
    nwg, lane_off, seg, tt = _plan(SHAPES[name][1])
    per_wg, (ctile, cblock) = LAYOUT[name]
    assert nwg == LANES and list(np.diff(lane_off)) == per_wg
    cut = [tuple(r) for r in seg if r[0] == ctile]
    assert cut == [(ctile, 0, cblock, 0), (ctile, cblock, tt[ctile], 1)] or cut == [(ctile, cblock, tt[ctile], 1), (ctile, 0, cblock, 0)]
    assert sum(1 for r in seg if r[1] > 0) == 1                                   # one cut
    assert tuple(seg[lane_off[0]]) == (ctile, 0, cblock, 0)                       # workgroup 0 starts with the cut tile's first blocks
    assert tuple(seg[lane_off[2] - 1]) == (ctile, cblock, tt[ctile], 1)           # workgroup 1 ends with its last blocks


@pytest.mark.parametrize("kw", KWS, ids=lambda k: "-".join("%s%g" % (a[:4], b) for a, b in k.items()) or "default")
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_lanes_equal_the_other_decoder_forms(eng, tables, name, kw):
    shape = SHAPES[name]
    mname, blocks, trunks, sig, off, ln = _group(eng, tables, shape)
    n = len(blocks)
    nwg, lane_off, seg, tt = _plan(blocks)
    p = eng.default_params(**kw)
    d = eng.upload(sig)
    st, calls = [], []
    try:
        eng.set_trunk_input(trunks)
        eng.debug_option("dump_final", 1)
        eng.debug_option("decoder_cus", 2)
        eng.debug_option("decoder_lanes", LANES)
        for sep, single in ((0, 0), (1, 0), (0, 1)):
            eng.debug_option("ff_separate", sep)
            eng.debug_option("fv_single", single)
            eng.run_device(d, off, ln, mname, p)
            calls.append(eng.collect(n, p))
            st.append(_tb_state(eng))
            nseg = int(eng.debug_fetch("decoder_pieces", np.int32)[0])
            nw = int(eng.debug_fetch("decoder_wgs", np.int32)[0])
            if (sep, single) == (0, 0):
                assert (nseg, nw) == (len(seg), LANES)              # the teams kernel: the planner's segments on two workgroups
            else:
                assert nseg == nw == 2 * len(tt)                    # the other two: two pieces a tile, a workgroup each
        codes = _same(st[0], st[1], calls[0], calls[1], blocks, "teams on lanes against k_ff_lds + k_viterbi in pieces")
        _same(st[0], st[2], calls[0], calls[2], blocks, "teams on lanes against k_ff_viterbi in pieces")
        if p.local_pen >= 100:
            assert np.mean(codes == 0) < 0.999                      # the traceback holds moves, not just stays
    finally:
        _reset(eng)
        eng.free(d)


def test_lanes_change_nothing(eng, tables):
    """the same group on whole tiles (five workgroups, a tile each) and on two lanes: identical"""
    shape = SHAPES["ragged"]
    mname, blocks, trunks, sig, off, ln = _group(eng, tables, shape)
    n = len(blocks)
    p = eng.default_params()
    d = eng.upload(sig)
    st, calls, shape_of = [], [], []
    try:
        eng.set_trunk_input(trunks)
        eng.debug_option("dump_final", 1)
        for lanes in (0, LANES):
            eng.debug_option("decoder_lanes", lanes)
            eng.run_device(d, off, ln, mname, p)
            calls.append(eng.collect(n, p))
            st.append(_tb_state(eng))
            shape_of.append((int(eng.debug_fetch("decoder_pieces", np.int32)[0]), int(eng.debug_fetch("decoder_wgs", np.int32)[0])))
        assert shape_of == [(5, 5), (6, 2)]
        _same(st[0], st[1], calls[0], calls[1], blocks, "whole tiles against two lanes")
    finally:
        _reset(eng)
        eng.free(d)
