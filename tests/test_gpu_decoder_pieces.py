"""The decoder's hand-over between the pieces of a tile, byte for byte, on small launch groups (run with -m gpu on an MI355X).

k_ff_viterbi_teams keeps the end state's score on one wave of its S1 team (producer 3 resolves the end state in phase B, sh_decode_teams.h:
per_read), the start state's score on the decoder threads, and a piece of a tile hands both to the next piece through the hand-over buffer by
two different routes.  Pieces normally need thousands of reads (more tiles than CUs); the debug option "decoder_cus" makes the piece schedule
believe in a device of that many CUs, so with 2 a group of three or five tiles is cut into two pieces a tile: ceil(T / 2) blocks and the rest.

The construction is test_gpu_decoder_bytes.py's (the logit table, one-hot trunk activations, the pinned tie columns: see there); every case
decodes one group with the teams kernel, with k_ff_lds + k_viterbi ("ff_separate") and with k_ff_viterbi ("fv_single") -- all three cut the same
way, the other two with their own, older hand-over -- and asks for identical traceback bytes of live states, end-state pointers, final states
and scores, the final scores of every state including the start / end slots, and the calls.

Shapes: 80 reads (five tiles) of one length, T = 3, 4, 5 (one-tap model) and 12 ... 17 (shipped geometry): odd and even lengths, a second piece
of one block (T = 3), piece boundaries on and off a boundary of the kernel's block pairs.  Ragged: one tile of reads of 3 ... 18 (12 ... 27)
blocks beside two tiles of the shortest reads (the engine sorts by length, so the sixteen longest reads make the first tile): its first piece is
9 (14) blocks, the reads shorter than that end inside it and their start / end scores must cross the hand-over unchanged."""
import numpy as np
import pytest

from scrappie_amd import synth
from test_gpu_decoder_bytes import NK, S, _same, _tb_state, _trunk, eng, tables  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CUS = 2                                                         # sh_pieces_per_tile(5, 2) = sh_pieces_per_tile(3, 2) = 2 (sh_sched.h)

# (model, block counts of the reads, kind of each read: 0 flat, 1 tied, 2 clear, 3 alternating).  One length: tiles of one kind each and a
# fifth tile of all four; ragged: kinds in turn
_MIX = [i // 16 if i < 64 else i % 4 for i in range(80)]
_TURN = [i % 4 for i in range(48)]
SHAPES = ([("tab1", [T] * 80, _MIX) for T in (3, 4, 5)] + [("tab5", [T] * 80, _MIX) for T in (12, 13, 14, 15, 16, 17)]
          + [("tab1", list(range(3, 19)) + [3] * 32, _TURN), ("tab5", list(range(12, 28)) + [12] * 32, _TURN)])
KWS = [dict(), dict(local_pen=150.0), dict(local_pen=150.0, min_prob=0.0), dict(skip_pen=0.25, stay_pen=0.1)]


def _group(eng, tables, shape):
    name, blocks, kinds = shape
    stride = tables[name]
    lens = [T * stride for T in blocks]
    assert [eng.read_blocks(name, ln) for ln in lens] == blocks
    sigs = [synth.medmad_normalise(synth.synthetic_signal(ln, 300 + i)) for i, ln in enumerate(lens)]
    # the first four tied reads are pinned to the tie columns 1 .. 4 (column 4: the end-state maximum twice in one quad and in a quad of another wave)
    tied_no = np.cumsum([k == 1 for k in kinds])
    pins = [int(tied_no[i]) if kinds[i] == 1 and tied_no[i] <= 4 else 0 for i in range(len(blocks))]
    assert sorted(p for p in pins if p) == [1, 2, 3, 4]
    trunks = [_trunk(T, kinds[i], 1000 * T + i, pins[i]) for i, T in enumerate(blocks)]
    ln = np.array(lens, np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]).astype(np.uint64)
    return name, blocks, trunks, np.concatenate(sigs), off, ln


def _reset(eng):
    for k in ("ff_separate", "fv_single", "dump_final", "decoder_cus"):
        eng.debug_option(k, 0)
    eng.set_trunk_input(None)


@pytest.mark.parametrize("kw", KWS, ids=lambda k: "-".join("%s%g" % (a[:4], b) for a, b in k.items()) or "default")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-T%d%s" % (s[0], s[1][0], "" if len(set(s[1])) == 1 else "to%d" % max(s[1])))
def test_two_pieces_equal_the_other_decoder_forms(eng, tables, shape, kw):
    name, blocks, trunks, sig, off, ln = _group(eng, tables, shape)
    n = len(blocks)
    p = eng.default_params(**kw)
    d = eng.upload(sig)
    st, calls = [], []
    try:
        eng.set_trunk_input(trunks)
        eng.debug_option("dump_final", 1)
        eng.debug_option("decoder_cus", CUS)
        for sep, single in ((0, 0), (1, 0), (0, 1)):
            eng.debug_option("ff_separate", sep)
            eng.debug_option("fv_single", single)
            eng.run_device(d, off, ln, name, p)
            calls.append(eng.collect(n, p))
            st.append(_tb_state(eng))
            assert int(eng.debug_fetch("decoder_pieces", np.int32)[0]) == 2 * ((n + 15) // 16)
        codes = _same(st[0], st[1], calls[0], calls[1], blocks, "teams against k_ff_lds + k_viterbi, two pieces a tile")
        _same(st[0], st[2], calls[0], calls[2], blocks, "teams against k_ff_viterbi, two pieces a tile")
        if p.local_pen >= 100:
            assert np.mean(codes == 0) < 0.999                  # the traceback holds moves, not just stays
    finally:
        _reset(eng)
        eng.free(d)


def test_the_option_cuts_every_tile_in_two_and_changes_nothing(eng, tables):
    """the launch count says the hand-over was exercised: 5 workgroups without the option, 10 with it; and one tile in one piece
    gives what two pieces give"""
    name, blocks, trunks, sig, off, ln = _group(eng, tables, SHAPES[5])
    n = len(blocks)
    p = eng.default_params()
    d = eng.upload(sig)
    st, calls, nwg = [], [], []
    try:
        eng.set_trunk_input(trunks)
        eng.debug_option("dump_final", 1)
        for cus in (0, CUS):
            eng.debug_option("decoder_cus", cus)
            eng.run_device(d, off, ln, name, p)
            calls.append(eng.collect(n, p))
            st.append(_tb_state(eng))
            nwg.append(int(eng.debug_fetch("decoder_pieces", np.int32)[0]))
        assert nwg == [5, 10]
        _same(st[0], st[1], calls[0], calls[1], blocks, "whole tiles against two pieces a tile")
    finally:
        _reset(eng)
        eng.free(d)
