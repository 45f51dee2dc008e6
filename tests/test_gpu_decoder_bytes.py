"""The decoder team's bookkeeping, byte for byte (run with -m gpu on an MI355X).

k_ff_viterbi_teams builds a quad's traceback codes, their store address, the one-addition path's test and the end-state scan
with as few instructions as it can; k_ff_lds + k_viterbi ("ff_separate") and k_ff_viterbi ("fv_single") do the same work the
plain way.  Every case here decodes ONE small launch group with all three and asks for identical traceback bytes, end-state
pointers, final states and scores of every live block; on the tiles of one length a sample of the reads is also decoded by the
oracle's decode_transducer on the engine's own posterior.

The posteriors are chosen, not random: the output layer is a table of 96 logit columns (ff_W[:, k], zero bias) and a read's
trunk activations are one-hot rows (scrappie_hip_set_trunk_input), so block t of a read has exactly the posterior of column
k_t, and states with equal logits have bit-identical posteriors:
  column 0        exactly flat (every move into every state ties; the end-state maximum is attained in every quad)
  column 1        two prefixes of one suffix are the best states: the step maximum is attained twice (first prefix wins)
  column 2        two skip prefixes r = 4 r4 + rl of one suffix tie
  column 3        the best step predecessor and the best skip predecessor of a quad tie (stay < step < skip: strict <)
  column 4        the end-state maximum in two states of one quad and in a quad of another wave
  columns 5-15    three logit levels at random: ties and near-ties everywhere
  columns 16-95   continuous logits: a clear runner-up, the one-addition path
The first four tied reads of a group are pinned: columns 0, c, 0, 0, c, 0, ... for c = 1 .. 4, so that the tie column c was built for is exact
(behind a flat block all scores are equal, and flat blocks keep the raised states equal): not left to the draw.
Reads of four kinds share a launch group -- flat, tied (columns 0-15), clear (16-95), alternating -- so a wave sees reads with a
clear runner-up beside reads without (the one-addition path's test is a vote of the wave), and tiles where every read has one.

Block counts: a tile of T blocks for T on both sides of every pair boundary.  The engine refuses reads below the model's
min_samples (the reference's edge arithmetic and gru_forward's two columns: 60 samples = 12 blocks for the shipped window of 19
at stride 5, 3 samples = 3 blocks for a one-tap window at stride 1), so T = 1 and T = 2 cannot be fed to any decoder form;
the cases are T = 3, 4, 5, 17 (one-tap model) and T = 12 ... 17 (shipped geometry).  Ragged tiles: 16 reads of 3 ... 18 and of
3 ... 33 blocks in steps of 2, 12 ... 27 and 12 ... 42 -- reads past their end keep their scores while the tile goes on.
No debug option cuts a tile into pieces without thousands of reads: pieces stay with test_gpu_parity.py's 4200-read groups."""
import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth

pytestmark = pytest.mark.gpu

NK, NS, S = 1024, 1025, 96


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


# the states columns 1 .. 4 raise
PIN_STATES = {1: [1 * 256 + 37, 3 * 256 + 37],                  # step into quad 37 from prefixes r4 = 1 and 3
              2: [2 * 64 + 9, 9 * 64 + 9],                      # skip into quads 36 .. 39 from r = 2 and 9
              3: [1 * 256 + 37, 5 * 64 + 9],                    # step and skip into quad 37
              4: [4 * 10 + 1, 4 * 10 + 3, 4 * 14 + 0]}          # quad 10 (wave 2) twice, quad 14 (wave 3)


def _logit_table():
    """(96, 1025): the logit columns of the module docstring"""
    rng = np.random.RandomState(77)
    P = np.zeros((S, NS), np.float32)
    for c, states in PIN_STATES.items():
        P[c, states] = 4.0
    for k in range(5, 16):
        P[k] = rng.choice(np.array([0.0, 2.0, 4.0], np.float32), size=NS, p=[0.9, 0.08, 0.02])
    P[16:] = rng.normal(0.0, 0.5, size=(S - 16, NS)).astype(np.float32)
    return P


@pytest.fixture(scope="module")
def tables(eng):
    """model name -> stride; both models share the logit table"""
    P = _logit_table()
    out = {}
    for name, kw in (("tab5", dict()), ("tab1", dict(winlen=1, stride=1))):
        w = model.synthetic_model("rgrgr_r94", seed=21, **kw)
        w["ff_W"] = np.ascontiguousarray(P.T)
        w["ff_b"] = np.zeros(NS, np.float32)
        eng.load_model(name, w)
        out[name] = int(w["stride"])
    return out


def _trunk(T, kind, seed, pin=0):
    """one-hot activations (T, 96) of a read of `kind`: 0 flat, 1 tied, 2 clear, 3 alternating tied / clear blocks.
    pin = c in 1 .. 4 (a tied read): columns 0, c, 0, 0, c, 0, ... -- behind an exactly flat block the states column c raises have
    bit-identical scores, and flat blocks and further blocks of column c keep them identical, so the tie c was built for is exact in every block
    from the third on (column 4: the end-state maximum in two states of quad 10 and in quad 14 of another wave, at every block)"""
    rng = np.random.RandomState(seed)
    tied = np.where(rng.rand(T) < 0.3, 0, rng.randint(0, 16, size=T))
    if pin:
        tied = np.where(np.arange(T) % 3 == 1, pin, 0)
    clear = rng.randint(16, S, size=T)
    col = [np.zeros(T, np.int64), tied, clear, np.where(np.arange(T) % 2 == 0, tied, clear)][kind]
    x = np.zeros((T, S), np.float32)
    x[np.arange(T), col] = 1.0
    return x


def _tb_state(eng):
    return {k: eng.debug_fetch(k, dt) for k, dt in (("tb", np.uint8), ("tb_end", np.int32), ("final_state", np.int32),
                                                   ("final_score", np.uint32), ("final_scores", np.uint32),
                                                   ("order", np.int32), ("tile_boff", np.int64))}


def _live_mask(st, blocks):
    """[column block][16] True where the block belongs to a read (t < its block count); `blocks` by call index"""
    order = st["order"]
    ntile = len(order) // 16
    rT = np.where(order >= 0, np.asarray(blocks)[np.maximum(order, 0)], 0).reshape(ntile, 16)
    boff = st["tile_boff"]
    ncb = len(st["tb_end"]) // 16
    live = np.zeros((ncb, 16), bool)
    for t in range(ntile):
        Tt = int(rT[t].max())
        live[boff[t]:boff[t] + Tt] = np.arange(Tt)[:, None] < rT[t][None, :]
    return live


def _same(a, b, ca, cb, blocks, what):
    assert np.array_equal(a["order"], b["order"]) and np.array_equal(a["tile_boff"], b["tile_boff"])
    live = _live_mask(a, blocks)
    ncb = live.shape[0]
    assert len(a["tb"]) == ncb * NK * 16
    ta, tb = a["tb"].reshape(ncb, 256, 16, 4), b["tb"].reshape(ncb, 256, 16, 4)
    m = np.broadcast_to(live[:, None, :, None], ta.shape)
    assert np.array_equal(ta[m], tb[m]), "traceback bytes differ: " + what      # (the whole byte of every live state: a select, not `& mask`)
    assert np.array_equal(a["tb_end"].reshape(ncb, 16)[live], b["tb_end"].reshape(ncb, 16)[live]), what
    real = a["order"] >= 0
    assert np.array_equal(a["final_state"][real], b["final_state"][real]), what
    assert np.array_equal(a["final_score"][real], b["final_score"][real]), what
    ntile = len(a["order"]) // 16
    fa, fb = a["final_scores"].reshape(ntile, NK * 16 + 32), b["final_scores"].reshape(ntile, NK * 16 + 32)
    rm = np.repeat(real.reshape(ntile, 1, 16), 256, axis=1)[..., None].repeat(4, axis=3).reshape(ntile, -1)
    assert np.array_equal(fa[:, :NK * 16][rm], fb[:, :NK * 16][rm]), "final scores of the k-mer states differ: " + what
    r2 = np.concatenate([real.reshape(ntile, 16)] * 2, axis=1)
    assert np.array_equal(fa[:, NK * 16:][r2], fb[:, NK * 16:][r2]), "start / end state scores differ: " + what
    key = lambda c: None if c is None else (c["bases"], c["score"], c["nblock"])
    assert [key(c) for c in ca] == [key(c) for c in cb], what
    return ta[m]


# a launch group: (model, block counts of its reads).  One length: 64 reads = 16 of each kind; ragged: 16 reads, kinds in turn
SHAPES = ([("tab1", [T] * 64) for T in (3, 4, 5, 17)] + [("tab5", [T] * 64) for T in (12, 13, 14, 15, 16, 17)]
          + [("tab1", list(range(3, 19))), ("tab1", list(range(3, 34, 2))), ("tab5", list(range(12, 28))), ("tab5", list(range(12, 43, 2)))])
# both template forms (skip_pen = 0 and not), a cheap and an expensive start / end state, min_prob at its default and at 0
# (no bound on |log-posterior|: the one-addition path is never taken)
KWS = [dict(), dict(local_pen=150.0), dict(local_pen=150.0, skip_pen=0.25), dict(skip_pen=0.25, stay_pen=0.1), dict(local_pen=150.0, min_prob=0.0)]


@pytest.mark.parametrize("kw", KWS, ids=lambda k: "-".join("%s%g" % (a[:4], b) for a, b in k.items()) or "default")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-T%d%s" % (s[0], s[1][0], "" if len(set(s[1])) == 1 else "to%d" % s[1][-1]))
def test_teams_bytes_equal_two_kernel_form_and_oracle(eng, orc, tables, shape, kw):
    name, blocks = shape
    stride = tables[name]
    n = len(blocks)
    kinds = [i // 16 if n == 64 else i % 4 for i in range(n)]
    lens = [T * stride for T in blocks]
    assert [eng.read_blocks(name, ln) for ln in lens] == blocks
    sigs = [synth.medmad_normalise(synth.synthetic_signal(ln, 300 + i)) for i, ln in enumerate(lens)]
    # the first four tied reads are pinned to columns 1 .. 4 (reads 16 .. 19 of 64; reads 1, 5, 9, 13 of a ragged tile)
    tied_no = np.cumsum([k == 1 for k in kinds])
    pins = [int(tied_no[i]) if kinds[i] == 1 and tied_no[i] <= 4 else 0 for i in range(n)]
    trunks = [_trunk(T, kinds[i], 1000 * T + i, pins[i]) for i, T in enumerate(blocks)]
    p = eng.default_params(**kw)
    ln = np.array(lens, np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]).astype(np.uint64)
    d = eng.upload(np.concatenate(sigs))
    st, calls = [], []
    try:
        eng.set_trunk_input(trunks)
        eng.debug_option("dump_final", 1)
        for sep, single in ((0, 0), (1, 0), (0, 1)):
            eng.debug_option("ff_separate", sep)
            eng.debug_option("fv_single", single)
            eng.run_device(d, off, ln, name, p)
            calls.append(eng.collect(n, p))
            st.append(_tb_state(eng))
        eng.debug_option("ff_separate", 0)
        eng.debug_option("fv_single", 0)
        eng.debug_option("dump_final", 0)
        codes = _same(st[0], st[1], calls[0], calls[1], blocks, "teams against k_ff_lds + k_viterbi")
        _same(st[0], st[2], calls[0], calls[2], blocks, "teams against k_ff_viterbi")
        if p.local_pen >= 100:
            assert np.mean(codes == 0) < 0.999              # the traceback holds moves, not just stays
        if n == 64:
            # the oracle on the engine's own posterior (decode.c:123, homopolymer.c:175, decode.c:449): four reads of every kind
            for i in sorted(set(range(0, n, 4)) | {j for j in range(n) if pins[j]}):
                eng.set_trunk_input([trunks[i]])
                post = eng.posterior(sigs[i], name, min_prob=p.min_prob)
                assert post.shape == (blocks[i], NS)
                if kinds[i] == 0:
                    assert np.all(post == post[0, 0])      # exactly flat
                if pins[i]:                                # the raised states really tie, above everything else, behind a flat block
                    top = PIN_STATES[pins[i]]
                    assert np.all(post[0] == post[0, 0]) and np.all(post[1, top] == post[1].max())
                    assert np.sum(post[1] == post[1].max()) == len(top)
                wsc, wseq = orc.decode_transducer(post, p.stay_pen, p.skip_pen, p.local_pen, False)
                if p.homopolymer:
                    rc, wseq = orc.homopolymer_path(post, wseq)
                wb, wpos = orc.overlapper(wseq, NK)
                c = calls[0][i]
                assert (c["bases"] if c else None) == wb, (i, kinds[i])
                if c:
                    assert np.float32(c["score"]) == np.float32(wsc) and c["nblock"] == blocks[i]
    finally:
        eng.debug_option("ff_separate", 0)
        eng.debug_option("fv_single", 0)
        eng.debug_option("dump_final", 0)
        eng.set_trunk_input(None)
        eng.free(d)
