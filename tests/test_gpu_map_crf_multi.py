"""One read of a flip-flop (CRF) model against many candidate sequences on the GPU (k_map_crf_pack, sh_map_crf_pack.h): the per-read
surface (scrappie_hip_map_trans_multi, sa.map_trans_to_sequences) on host-made matrices against the numpy restatement and this
library's own map_crf_to_sequence_* candidate by candidate; Engine.map_to_sequences_crf against Engine.map_to_sequence with every
read repeated once per candidate; `scrappie seqmappy --each-record`.  Scores are bit-identical, Viterbi and forward (the same
per-cell function in the same order); forward also meets the project's criterion against float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_gpu_map_crf import _HostMat, _prepared, gpu_map
from test_map_crf_cpu import _trans, call_of, crf_lds_max_seq, np_decode_crf, np_map_crf, ref_decode_crf
from test_map_crf_multi_cpu import ranking_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
READS = os.path.join(ROOT, "tests", "golden", "reads")
READ = "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand"
NO_PATH = "no admissible path"


@pytest.fixture(scope="module", autouse=True)
def pack_forms_at_start():
    """k_map_crf_pack launches per form before this module's first test (test_every_pack_form_was_launched)"""
    return sa.map_crf_pack_form_counts()


@pytest.fixture(autouse=True)
def default_pack_cells():
    """every test leaves the per-read surface's engine at the default pack size"""
    yield
    sa.set_map_crf_pack_cells(-1)


def trans_multi(trans, cands, viterbi, stride=28, bands=None):
    """scrappie_hip_map_trans_multi on a numpy [nblock][25] matrix and base-code arrays: (rc, float32 scores)"""
    m = _HostMat(np.ascontiguousarray(trans, dtype=np.float32), stride)
    keep = [np.ascontiguousarray(c, dtype=np.int32) for c in cands]
    tgs = (sa._MapTarget * max(len(keep), 1))()
    edges = []
    for i, c in enumerate(keep):
        tgs[i].seq = c.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(c)
        if bands and i in bands:
            lo, hi = (np.ascontiguousarray(b, dtype=np.uintp) for b in bands[i])
            edges += [lo, hi]
            tgs[i].poslow = lo.ctypes.data_as(C.POINTER(C.c_size_t))
            tgs[i].poshigh = hi.ctypes.data_as(C.POINTER(C.c_size_t))
    score = np.full(len(cands), 7.0, dtype=np.float32)
    rc = sa.lib().scrappie_hip_map_trans_multi(C.byref(m.mat), tgs, len(cands), 1 if viterbi else 0, score.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, score


def multi(trans, cands, viterbi, stride=28):
    rc, score = trans_multi(trans, cands, viterbi, stride)
    assert rc == 0, sa.last_error()
    return score


def single(trans, cands, viterbi, stride=28):
    """this library's own map_crf_to_sequence_viterbi / _forward, candidate by candidate (k_map_crf)"""
    return np.array([gpu_map(trans, c, viterbi=viterbi, stride=stride)[0] for c in cands], dtype=np.float32)


def np_scores(trans, cands, viterbi=True, dtype=np.float32):
    return np.array([np_map_crf(trans, c, viterbi=viterbi, dtype=dtype)[0] for c in cands], dtype=dtype)


def _rand(rng, n):
    return rng.integers(0, 4, n).astype(np.int32)


def _same(a, b):
    """the same float32 bits, a NaN being any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()


def _forward_ok(got, np32, f64, what):
    for g, r, x in zip(got, np32, f64):
        if np.isnan(x):
            assert np.isnan(g), what
            continue
        print("forward %s: gpu %.9g np32 %.9g f64 %.12g" % (what, g, r, x))
        assert abs(float(g) - float(x)) <= 2 * abs(float(r) - float(x)) + 1e-5 * abs(float(x)), (what, g, r, x)


# ---------------------------------------------------------------------------
# host-made matrices
# ---------------------------------------------------------------------------
def test_cell_kinds_and_segment_boundaries():
    """candidates of 1, 3, 2, 18 (the only path), 19 (no path), 1 and 2 bases in one pack against 17 blocks: every cell kind directly
    beside every other across a segment boundary"""
    rng = np.random.default_rng(71)
    trans = _trans(17, 2.0, rng)
    cands = [_rand(rng, n) for n in (1, 3, 2, 18, 19, 1, 2)]
    assert sa.map_crf_pack_plan([len(c) for c in cands], 512)[2] == 1
    before = sa.map_crf_pack_form_counts()
    got_v = multi(trans, cands, True)
    assert NO_PATH in sa.last_error() and "candidate 4" in sa.last_error()
    want_v = np_scores(trans, cands)
    assert np.isnan(got_v[4]) and np.isnan(want_v[4]) and np.all(np.isfinite(np.delete(got_v, 4)))
    assert _same(got_v, want_v), (got_v, want_v)
    assert _same(got_v, single(trans, cands, True)), got_v
    got_f = multi(trans, cands, False)
    assert _same(got_f, single(trans, cands, False)), got_f
    _forward_ok(got_f, np_scores(trans, cands, False), np_scores(trans, cands, False, np.float64), "kinds")
    after = sa.map_crf_pack_form_counts()
    assert after[(True, False)] - before[(True, False)] == 1 and after[(False, False)] - before[(False, False)] == 1
    for vit, first in ((True, got_v), (False, got_f)):
        assert _same(multi(trans, cands[::-1], vit), first[::-1]), vit
        for k, c in enumerate(cands):
            assert _same(multi(trans, [c], vit), first[k:k + 1]), (vit, k)


@pytest.mark.parametrize("stride", [25, 28])
def test_prefetch_ring_edges(stride):
    """reads of 1, 2, 3, 4, 5 and 9 blocks: fewer columns than are in flight (SH_MAPC_D = 4), exactly as many, one more, and two
    rounds plus one"""
    rng = np.random.default_rng(73 + stride)
    for nb in (1, 2, 3, 4, 5, 9):
        trans = _trans(nb, 2.0, rng)
        cands = [_rand(rng, n) for n in sorted({1, 2, max(1, nb // 2), nb, nb + 1})] + [_rand(rng, 1)]
        got_v = multi(trans, cands, True, stride)
        assert np.all(np.isfinite(got_v)) and _same(got_v, np_scores(trans, cands)), (nb, got_v)
        got_f = multi(trans, cands, False, stride)
        assert _same(got_f, single(trans, cands, False, stride)), (nb, got_f)
        _forward_ok(got_f, np_scores(trans, cands, False), np_scores(trans, cands, False, np.float64), "nb%d" % nb)


@pytest.fixture(scope="module")
def long_trans():
    return _trans(510, 2.0, np.random.default_rng(79))


@pytest.mark.parametrize("cells", [[200, 55], [254, 2], [255, 2], [256, 255, 2]])
def test_chunks_of_threads(cells, long_trans):
    """packs of 255, 256, 257 and 513 cells (one, one, two and three chunks of 256 threads): a candidate that ends on thread 255, one
    that lies across threads 255 | 256, one that begins on thread 0 of the second chunk; a read of twice the longest's bases"""
    rng = np.random.default_rng(sum(cells))
    cands = [_rand(rng, c - 1) for c in cells]
    sa.set_map_crf_pack_cells(sa.map_crf_pack_max_cells())
    assert sa.map_crf_pack_plan([len(c) for c in cands], sa.map_crf_pack_max_cells())[2] == 1
    assert long_trans.shape[0] == 2 * 255
    got_v = multi(long_trans, cands, True)
    assert np.all(np.isfinite(got_v)) and _same(got_v, np_scores(long_trans, cands)), got_v
    got_f = multi(long_trans, cands, False)
    assert _same(got_f, single(long_trans, cands, False)), got_f
    _forward_ok(got_f, np_scores(long_trans, cands, False), np_scores(long_trans, cands, False, np.float64), "cells%d" % sum(cells))


def test_ties():
    """all-zero transitions: every path of every candidate ties, a homopolymer among them; the bits of the restatement (the lowest
    index as `best` on a tie: test_engine_lanes_tiles_and_shared_sets, where a read has the same candidate three times)"""
    rng = np.random.default_rng(83)
    trans = np.zeros((20, 25), dtype=np.float32)
    cands = [_rand(rng, 7), np.full(5, 1, dtype=np.int32), _rand(rng, 7), _rand(rng, 21), np.full(1, 3, dtype=np.int32)]
    got_v = multi(trans, cands, True)
    assert _same(got_v, np_scores(trans, cands)) and np.all(got_v == 0), got_v
    got_f = multi(trans, cands, False)
    assert _same(got_f, single(trans, cands, False)), got_f
    _forward_ok(got_f, np_scores(trans, cands, False), np_scores(trans, cands, False, np.float64), "ties")


def test_pack_size_does_not_change_bits():
    rng = np.random.default_rng(89)
    trans = _trans(130, 2.0, rng)
    lens = [1, 120, 2, 3] + [int(x) for x in rng.integers(1, 121, 20)]
    cands = [_rand(rng, n) for n in lens]
    maxc = sa.map_crf_pack_max_cells()
    for vit in (True, False):
        got = {}
        for pc in (0, 64, 257, -1, maxc):
            sa.set_map_crf_pack_cells(pc)
            pb, fb = sa.map_crf_pack_form_counts()[(vit, False)], sa.map_crf_form_counts()[(vit, False, False)]
            got[pc] = multi(trans, cands, vit)
            pa, fa = sa.map_crf_pack_form_counts()[(vit, False)], sa.map_crf_form_counts()[(vit, False, False)]
            assert (pa - pb, fa - fb) == ((0, 1) if pc == 0 else (1, 0)), (vit, pc)
        assert all(np.all(np.isfinite(g)) and _same(g, got[0]) for g in got.values()), (vit, got)
    assert _same(got[0], single(trans, cands, False))


def test_oversize_candidate_takes_k_map_crf():
    """a candidate of max_cells bases -- one cell too many for any pack -- between two short ones, against max_cells + 2 blocks: it
    goes through k_map_crf (in its scratch home: longer than its LDS home holds) beside packed neighbours"""
    maxc = sa.map_crf_pack_max_cells()
    rng = np.random.default_rng(97)
    trans = _trans(maxc + 2, 2.0, rng)
    cands = [_rand(rng, 40), _rand(rng, maxc), _rand(rng, 7)]
    pack, _, npack = sa.map_crf_pack_plan([len(c) for c in cands], 512)
    assert pack.tolist() == [0, -1, 0] and npack == 1 and maxc > crf_lds_max_seq()
    for vit in (True, False):
        pb, fb = sa.map_crf_pack_form_counts()[(vit, False)], sa.map_crf_form_counts()
        got = multi(trans, cands, vit)
        pa, fa = sa.map_crf_pack_form_counts()[(vit, False)], sa.map_crf_form_counts()
        assert pa - pb == 1 and fa[(vit, False, True)] - fb[(vit, False, True)] == 1 and fa[(vit, False, False)] == fb[(vit, False, False)]
        assert np.all(np.isfinite(got)) and _same(got, single(trans, cands, vit)), (vit, got)
    assert _same(multi(trans, cands, True), np_scores(trans, cands))


def test_own_call_wins_through_map_trans_to_sequences():
    trans, cands, own_at = ranking_fixture()
    m = sa.ScrappyMatrix.from_numpy(trans, sloika=False)
    for vit in (True, False):
        s = sa.map_trans_to_sequences(m, cands, viterbi=vit)
        assert s.dtype == np.float32 and np.all(np.isfinite(s)) and int(np.argmax(s)) == own_at and np.sum(s == s[own_at]) == 1, (vit, s)
        if vit:
            ref = ref_decode_crf(trans)
            want = ref[0] if ref is not None else np_decode_crf(trans)[0]
            assert np.float32(s[own_at]).tobytes() == np.float32(want).tobytes(), (s[own_at], want)
    strings = ["".join("ACGT"[b] for b in c) for c in cands]
    assert _same(sa.map_trans_to_sequences(m, strings, viterbi=False), s)


# ---------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    return model.synthetic_model("rnnrf_r94", seed=11), model.synthetic_model("rgrgr_r94", seed=1)


@pytest.fixture(scope="module")
def eng(weights):
    e = sa.Engine(0)
    e.load_model("rnnrf_r94", weights[0])
    e.load_model("rgrgr_r94", weights[1])
    yield e
    e.close()


def _sig(n, seed):
    return synth.medmad_normalise(synth.synthetic_signal(n, seed))


def _bases(n, rng):
    return "".join(rng.choice(list("ACGT"), n))


def _repeated(eng, sigs, lists, **kw):
    """Engine.map_to_sequence with each read repeated once per candidate: [[(score, path)] per read]"""
    flat_s = [x for x, cl in zip(sigs, lists) for _ in cl]
    flat_q = [q for cl in lists for q in cl]
    res = eng.map_to_sequence(flat_s, flat_q, model="rnnrf_r94", **kw) if flat_s else []
    out, at = [], 0
    for cl in lists:
        out.append(res[at:at + len(cl)])
        at += len(cl)
    return out


def _best(scores):
    ok = np.isfinite(scores)
    return int(np.flatnonzero(ok & (scores == scores[ok].max()))[0]) if ok.any() else -1


def _check_against_repeated(got, want, path):
    assert len(got) == len(want)
    for i, ((sc, best, pth), w) in enumerate(zip(got, want)):
        ws = np.array([s for s, _ in w], dtype=np.float32)
        assert sc.dtype == np.float32 and _same(sc, ws), (i, sc, ws)
        assert best == _best(ws), (i, best, ws)
        if path and best >= 0:
            assert pth is not None and np.array_equal(pth, w[best][1]), i
        else:
            assert pth is None, i


@pytest.fixture(scope="module")
def engine_reads():
    rng = np.random.default_rng(37)
    lens = [int(x) for x in rng.integers(600, 1500, 18)]                       # two tiles, every lane index
    return [_sig(n, 800 + i) for i, n in enumerate(lens)]


def test_engine_lanes_tiles_and_shared_sets(eng, engine_reads):
    rng = np.random.default_rng(39)
    sigs = engine_reads
    nblock = [eng.read_blocks("rnnrf_r94", len(x)) for x in sigs]
    shared = [_bases(n, rng) for n in (44, 100, 9, 1, 44)]
    per_read = [[_bases(int(rng.integers(1, nb // 2)), rng) for _ in range(int(k))] for k, nb in zip(rng.integers(2, 7, len(sigs)), nblock)]
    per_read[4] = []                                                           # K = 0
    per_read[11] = [_bases(50, rng)]                                           # K = 1
    per_read[6] = [per_read[6][0]] * 3                                         # all tie: the lowest index wins
    per_read[8] = per_read[8] + [_bases(nblock[8] + 2, rng)]                   # more bases than entries: no admissible path
    for lists, arg in (([shared] * len(sigs), shared), (per_read, per_read)):
        for vit in (True, False):
            before = sa.map_crf_pack_form_counts()[(vit, True)]
            got = eng.map_to_sequences_crf(sigs, arg, viterbi=vit, path=vit)
            err = sa.last_error()
            assert sa.map_crf_pack_form_counts()[(vit, True)] == before + 1    # one launch for the group
            want = _repeated(eng, sigs, lists, viterbi=vit, path=vit)
            _check_against_repeated(got, want, vit)
            if vit:
                assert all(len(pth) == nb + 1 for (_, best, pth), nb in zip(got, nblock) if best >= 0)
    assert "read 8" in err and NO_PATH in err, err
    assert got[4][0].shape == (0,) and got[4][1] == -1 and got[6][1] == 0 and np.isnan(got[8][0][-1]) and got[8][1] >= 0
    t = eng.map_timing()
    assert t["network_ms"] > 0 and t["map_ms"] > 0
    # the route without packs: the network once, k_map_crf per candidate
    packed = eng.map_to_sequences_crf(sigs, per_read, viterbi=True, path=True)
    eng.debug_option("map_crf_pack_cells", 0)
    try:
        before = sa.map_crf_pack_form_counts()
        unpacked = eng.map_to_sequences_crf(sigs, per_read, viterbi=True, path=True)
        assert sa.map_crf_pack_form_counts() == before
    finally:
        eng.debug_option("map_crf_pack_cells", -1)
    for (a, ab, ap), (b, bb, bp) in zip(unpacked, packed):
        assert _same(a, b) and ab == bb and ((ap is None and bp is None) or np.array_equal(ap, bp))


def test_engine_own_call_wins(eng, engine_reads):
    """each read's own call -- decode_crf's path through call_of, so the base of its last entry is kept -- among decoys: it wins with
    decode_crf's score in bits"""
    rng = np.random.default_rng(41)
    sigs, lists, want = [], [], []
    for x in engine_reads[:8]:
        trans = eng.posterior(x, "rnnrf_r94")
        ref = ref_decode_crf(trans)
        ds, dp = ref if ref is not None else np_decode_crf(trans)
        own = call_of(dp)[0]
        if len(own) < 3:                                                       # (a call too short to edit)
            continue
        sigs.append(x)
        sub = own.copy()
        sub[len(own) // 2] = (sub[len(own) // 2] + 1 + rng.integers(0, 3)) % 4
        text = lambda c: "".join("ACGT"[b] for b in c)
        lists.append([_bases(len(own) // 2, rng), text(sub), text(own), text(np.delete(own, len(own) // 3)), _bases(len(own), rng)])
        want.append(np.float32(ds))
    assert len(sigs) >= 4
    got = eng.map_to_sequences_crf(sigs, lists, viterbi=True)
    for i, (sc, best, pth) in enumerate(got):
        assert best == 2 and np.sum(sc == sc[2]) == 1 and np.float32(sc[2]).tobytes() == want[i].tobytes(), (i, sc, want[i])


def test_engine_launch_groups_cut_by_memory(eng):
    """launch groups cut by device bytes as test_engine_map_multi_cut_by_memory cuts them: a budget of 240 column blocks puts the reads
    of 200, 140, [300], 198 | 200, 120, 199 | 170 blocks into three groups and refuses the read of 300, which needs 319 alone;
    the others as in one uncut launch group, bit for bit"""
    lens = [1000, 700, 1500, 990, 1000, 600, 995, 850]
    rng = np.random.default_rng(51)
    sigs = [_sig(n, 400 + i) for i, n in enumerate(lens)]
    assert [eng.read_blocks("rnnrf_r94", n) for n in lens] == [200, 140, 300, 198, 200, 120, 199, 170]
    cands = [_bases(34, rng) for _ in range(3)]
    kw = dict(viterbi=True, path=True)
    before = sa.map_crf_pack_form_counts()[(True, True)]
    uncut = eng.map_to_sequences_crf(sigs, cands, **kw)
    assert sa.map_crf_pack_form_counts()[(True, True)] == before + 1
    assert all(np.all(np.isfinite(sc)) and best >= 0 and pth is not None for sc, best, pth in uncut)
    eng.set_max_launch_blocks(240)
    try:
        cut = eng.map_to_sequences_crf(sigs, cands, **kw)
        err = sa.last_error()
    finally:
        eng.set_max_launch_blocks(0)
    groups = sa.map_crf_pack_form_counts()[(True, True)] - before - 1
    print("launch groups under a budget of 240 blocks: %d" % groups)
    assert groups >= 3
    assert np.all(np.isnan(cut[2][0])) and len(cut[2][0]) == 3 and cut[2][1] == -1 and cut[2][2] is None
    assert "read 2" in err and "too long for one launch group" in err, err
    for i, ((a, ab, ap), (b, bb, bp)) in enumerate(zip(cut, uncut)):
        if i != 2:
            assert _same(a, b) and ab == bb and np.array_equal(ap, bp), i


def test_refusals(eng, engine_reads):
    rng = np.random.default_rng(43)
    sigs = engine_reads[:2]
    with pytest.raises(RuntimeError, match="rgrgr_r94.*transducer"):
        eng.map_to_sequences_crf(sigs, ["ACGTACGTAC"], model="rgrgr_r94")
    good = [_bases(40, rng), _bases(90, rng)]
    clean = eng.map_to_sequences_crf(sigs, good)
    got = eng.map_to_sequences_crf(sigs, [good[0], "", "ACGNT", good[1]])
    err = sa.last_error()
    assert "read 0" in err and "candidate 1" in err and "empty sequence" in err, err
    for (sc, best, _), (cs, cb, _) in zip(got, clean):
        assert np.isnan(sc[1]) and np.isnan(sc[2]) and _same(sc[[0, 3]], cs) and best == (0, 3)[cb]
    got = eng.map_to_sequences_crf([sigs[0], sigs[1][:5]], good)               # the second is below the model's minimum
    assert "read 1" in sa.last_error() and "too short" in sa.last_error()
    assert _same(got[0][0], clean[0][0]) and np.all(np.isnan(got[1][0])) and len(got[1][0]) == 2 and got[1][1] == -1
    # the per-read surface
    trans = _trans(30, 2.0, rng)
    cands = [_rand(rng, 5), np.array([0, 4, 1], dtype=np.int32), _rand(rng, 9)]
    alone = multi(trans, [cands[0], cands[2]], True)
    rc, s = trans_multi(trans, cands, True)
    assert rc == 0 and np.isnan(s[1]) and _same(s[[0, 2]], alone), s
    assert "candidate 1" in sa.last_error() and "code 4" in sa.last_error() and "not a base" in sa.last_error()
    lo, hi = sa.map_crf_diagonal_band(30, 9, 3)
    rc, s = trans_multi(trans, [cands[0], cands[2]], True, bands={1: (lo, hi)})
    assert rc == 0 and np.isnan(s[1]) and _same(s[:1], alone[:1]) and "candidate 1: bands are not part of this call" in sa.last_error()
    rc, s = trans_multi(trans, [cands[0], np.zeros(0, dtype=np.int32)], False)
    assert rc == 0 and np.isnan(s[1]) and np.isfinite(s[0]) and "candidate 1: an empty sequence" in sa.last_error()
    rc, s = trans_multi(trans, [], True)
    assert rc == 0 and s.shape == (0,)
    m = _HostMat(trans)
    out = np.full(2, 7.0, dtype=np.float32)
    assert sa.lib().scrappie_hip_map_trans_multi(C.byref(m.mat), None, 2, 1, out.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert "null argument" in sa.last_error()
    # a NULL cand with ncand > 0 through the batch call: that read is refused, its neighbour scored
    rts, keep = sa._raw_tables(sigs)
    tgs, kept = sa._crf_targets(good)
    cds = (sa._MapCandidates * 2)()
    cds[0].cand, cds[0].ncand = None, 2
    cds[1].cand, cds[1].ncand = tgs, 2
    p = eng.default_params()
    res = (sa._MapMultiResult * 2)()
    assert sa.lib().scrappie_hip_map_crf_multi_batch(eng._h, eng._models["rnnrf_r94"], rts, cds, 2, C.byref(p), 1, 0, res) == 0
    assert "read 0" in sa.last_error() and "no candidates" in sa.last_error()
    assert res[0].best == -1 and np.all(np.isnan(np.ctypeslib.as_array(res[0].score, shape=(2,))))
    assert _same(np.ctypeslib.as_array(res[1].score, shape=(2,)), clean[1][0]) and res[1].best == clean[1][1]
    sa.lib().scrappie_hip_free_map_multi_results(res, 2)


# ---------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------
def test_seqmappy_each_record(eng, weights, tmp_path):
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    trans = eng.posterior(x, "rnnrf_r94")
    ref = ref_decode_crf(trans)
    own = "".join("ACGT"[b] for b in call_of((ref if ref is not None else np_decode_crf(trans))[1])[0])
    rng = np.random.default_rng(61)
    recs = [("decoy_a", _bases(max(1, len(own) // 2), rng)), ("own_call", own), ("decoy_b", _bases(len(own), rng))]
    fa3 = tmp_path / "three.fa"
    fa3.write_text("".join(">%s some description\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in recs))
    crf_file, tr_file = str(tmp_path / "rnnrf_r94.scrm"), str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(weights[0], crf_file)
    model.save_model(weights[1], tr_file)
    (scores, best, path), = eng.map_to_sequences_crf([x], [s for _, s in recs], viterbi=True, path=True)
    nb = len(path) - 1
    assert best == 1 and nb == eng.read_blocks("rnnrf_r94", len(x))
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--each-record", str(fa3), f5], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "# %s to %s -- 3 records" % (f5, fa3) and lines[1] == "record\tname\tscore\tper_block"
    for k, (n, _) in enumerate(recs):
        assert lines[2 + k] == "%d\t%s\t%f\t%f" % (k, n, -scores[k], np.float32(-scores[k]) / np.float32(nb)), (k, lines[2 + k])
    # the record of the best: what plain seqmappy prints on a FASTA that holds only that record, under the name fasta:name
    fa1 = tmp_path / "one.fa"
    fa1.write_text(">%s\n%s\n" % recs[best])
    one = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, str(fa1), f5], capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr
    assert "\n".join(lines[5:]) + "\n" == one.stdout.replace(" to %s -- " % fa1, " to %s:%s -- " % (fa3, recs[best][0]), 1)
    assert len(lines) == 5 + 2 + nb + 1
    # what stops before anything runs
    bad = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--each-record", str(fa3), f5], capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--each-record" in bad.stderr and "--all-records" in bad.stderr and "rgrgr_r94" in bad.stderr and bad.stdout == ""
    for other in ("--all-records", "--inside", "--find", "--within"):
        bad = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--each-record", other, str(fa3), f5], capture_output=True, text=True, timeout=60)
        assert bad.returncode != 0 and "--each-record" in bad.stderr and other in bad.stderr and bad.stdout == "", other
    bad = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--all-records", str(fa3), f5], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--all-records" in bad.stderr and bad.stdout == ""
    u = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    assert "--each-record" in u.stderr + u.stdout


def test_every_pack_form_was_launched(pack_forms_at_start):
    """the last test of the module: each of the four k_map_crf_pack instantiations (Viterbi / forward x reference layout / tiled) has
    been launched by the tests above"""
    now = sa.map_crf_pack_form_counts()
    ran = {k: now[k] - pack_forms_at_start[k] for k in now}
    print("k_map_crf_pack launches by (viterbi, tiled): %r" % sorted(ran.items()))
    assert len(ran) == 4 and all(v > 0 for v in ran.values()), ran
