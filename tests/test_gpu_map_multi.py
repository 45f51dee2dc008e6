"""One read against many candidate sequences on the GPU (k_map_pack, sh_map_pack.h): the per-read surface
(scrappie_hip_map_post_multi, sa.map_post_to_sequences) against the compiled reference, the numpy restatement and this
library's own map_to_sequence_* candidate by candidate; Engine.map_to_sequences against Engine.map_to_sequence with every
read repeated once per candidate; `scrappie seqmappy --all-records`.  Scores are bit-identical, Viterbi and forward (the same
per-cell function in the same order); forward also meets tests/test_gpu_map.py's criterion against float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import scrappie_amd as sa
from scrappie_amd import model, synth
from test_map_cpu import call_map, lds_max_seq, np_map, ref_decode_lib
from test_map_multi_cpu import winner_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
READS = os.path.join(ROOT, "tests", "golden", "reads")
PM = C.POINTER(sa._Mat)
NK = 64                                     # k = 3 posteriors for the per-read cases
PEN0, PEN150 = (0.0, 0.0, 4.0), (150.0, 150.0, 120.0)


@pytest.fixture(scope="module")
def ref():
    R = ref_decode_lib()
    assert R is not None, "oracle/_ref/libref_decode.so is required (build() makes it and it travels with the tree)"
    return R


@pytest.fixture(scope="module", autouse=True)
def pack_forms_at_start():
    """k_map_pack launches per form before this module's first test (test_every_pack_form_was_launched)"""
    return sa.map_pack_form_counts()


@pytest.fixture(autouse=True)
def default_pack_cells():
    """every test leaves the per-read surface's engine at the default pack size"""
    yield
    sa.set_map_pack_cells(-1)


def post_multi(post, cands, pens, viterbi):
    """scrappie_hip_map_post_multi on a numpy posterior and state-code arrays: float32 scores"""
    m = oracle.NpMat(post)
    keep = [np.ascontiguousarray(c, dtype=np.int32) for c in cands]
    tgs = (sa._MapTarget * max(len(keep), 1))()
    for i, c in enumerate(keep):
        tgs[i].seq = c.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(c)
    score = np.full(len(keep), 7.0, dtype=np.float32)
    rc = sa.lib().scrappie_hip_map_post_multi(C.cast(m.ptr, PM), *pens, tgs, len(keep), 1 if viterbi else 0, score.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0, sa.last_error()
    return score


def single(post, cands, pens, viterbi):
    """this library's own map_to_sequence_viterbi / _forward, candidate by candidate (k_map)"""
    return np.array([call_map(sa.lib(), post, c, pens, viterbi, cast=PM)[0] for c in cands], dtype=np.float32)


def _rand(rng, n):
    return rng.integers(0, NK, n).astype(np.int32)


def _true(tpath, rng):
    s = [int(x) for x in tpath if x >= 0]
    return np.array(s if len(s) >= 3 else rng.integers(0, NK, 3), dtype=np.int32)


def parity_cases():
    """(name, post, candidates, pens): k = 3 posteriors of 1, 2, 41 and 800 blocks and a flat one; the candidate lists of the issue"""
    rng = np.random.default_rng(17)
    posts = {T: synth.simulated_posterior(T, 300 + T, klen=3) for T in (1, 2, 41, 800)}
    out = []
    for j, T in enumerate((1, 2, 41, 800)):
        post, tpath = posts[T]
        mixed = [_rand(rng, n) for n in (1, 2, 3, 40, 300, 2, 1, 3)]          # the position 0 / 1 / >= 2 branches beside long ones
        out.append(("T%d_mixed_pen0" % T, post, mixed, PEN0))
        out.append(("T%d_mixed_pen150" % T, post, mixed, PEN150))
        out.append(("T%d_K1" % T, post, [_rand(rng, 40)], (PEN0, PEN150)[j % 2]))
    post, tpath = posts[800]
    true = _true(tpath, rng)
    # totals of 63 ... 2 x 256 + 1 cells: the last candidate ends at the total, and a candidate lies across cells 63 | 64, 255 | 256, 511 | 512
    for j, total in enumerate((63, 64, 65, 255, 256, 257, 2 * 256 + 1)):
        lens = [28, total - 32] if total < 300 else [28, 200, total - 30 - 202 - 2]
        assert sum(n + 2 for n in lens) == total
        out.append(("cells%d" % total, posts[(41, 800)[j % 2]][0], [_rand(rng, n) for n in lens], (PEN0, PEN150)[j % 2]))
    # a perfect match directly before and directly after a candidate that does not match: a leak across a segment boundary
    # (step, skip, START or END read from the neighbour) would raise the neighbour's score
    other = _rand(rng, len(true))
    out.append(("match_nomatch_match", post, [true, other, true], PEN0))
    out.append(("nomatch_match_nomatch", post, [other, true, other[:-5]], PEN0))
    flat = synth.fixture_posterior(41, 5, klen=3, hp=-1)                       # everything ties
    out.append(("flat_pen0", flat, [_rand(rng, n) for n in (1, 2, 3, 40, 300, 40)], PEN0))
    out.append(("flat_pen150", flat, [_rand(rng, n) for n in (3, 40, 2, 41)], PEN150))
    return out


@pytest.fixture(scope="module")
def parity(ref):
    """parity_cases with what the reference and the restatements give, computed once"""
    out = []
    for name, post, cands, pens in parity_cases():
        c = dict(name=name, post=post, cands=cands, pens=pens)
        c["ref_v"] = np.array([call_map(ref, post, s, pens, True)[0] for s in cands], dtype=np.float32)
        c["np_v"] = np.array([np.float32(np_map(post, s, *pens)[0]) for s in cands], dtype=np.float32)
        c["ref_f"] = np.array([call_map(ref, post, s, pens, False)[0] for s in cands], dtype=np.float32)
        c["f64"] = [float(np_map(post, s, *pens, viterbi=False, dtype=np.float64)[0]) for s in cands]
        out.append(c)
    return out


def test_per_read_parity_dense(parity):
    maxc = sa.map_pack_max_cells()
    sa.set_map_pack_cells(maxc)                      # every list in one pack: the boundaries the lists are built around are inside it
    before = sa.map_pack_form_counts()
    worst = 0.0
    for c in parity:
        name, post, cands, pens = c["name"], c["post"], c["cands"], c["pens"]
        got_v = post_multi(post, cands, pens, True)
        own_v = single(post, cands, pens, True)
        assert got_v.tobytes() == c["ref_v"].tobytes(), (name, got_v, c["ref_v"])
        assert got_v.tobytes() == c["np_v"].tobytes(), (name, got_v, c["np_v"])
        assert got_v.tobytes() == own_v.tobytes(), (name, got_v, own_v)
        got_f = post_multi(post, cands, pens, False)
        own_f = single(post, cands, pens, False)
        assert got_f.tobytes() == own_f.tobytes(), (name, got_f, own_f)
        for g, r, x in zip(got_f, c["ref_f"], c["f64"]):
            eg, er = abs(float(g) - x), abs(float(r) - x)
            assert eg <= 2 * er + 1e-5 * abs(x), (name, g, r, x)
            worst = max(worst, eg / (er + 1e-5 * abs(x) + 1e-30))
    after = sa.map_pack_form_counts()
    assert after[(True, False)] - before[(True, False)] == len(parity) and after[(False, False)] - before[(False, False)] == len(parity)
    print("forward: worst |gpu - f64| / (|ref - f64| + 1e-5 |score|) = %.3f" % worst)


def test_scrappy_style_map_post_to_sequences(ref):
    """the Python surface on base strings: the scores of map_post_to_sequence one by one, NaN for a sequence that cannot be encoded"""
    post, _ = synth.simulated_posterior(300, 4, klen=3)
    rng = np.random.default_rng(4)
    seqs = ["".join(rng.choice(list("ACGT"), n)) for n in (200, 12, 3, 77)]
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    for vit in (True, False):
        got = sa.map_post_to_sequences(m, seqs + ["ACGNT"], viterbi=vit)
        assert got.dtype == np.float32 and got.shape == (5,) and np.isnan(got[4])
        want = np.array([sa.map_post_to_sequence(m, s, viterbi=vit)[0] for s in seqs], dtype=np.float32)
        assert got[:4].tobytes() == want.tobytes(), (vit, got, want)
    assert "candidate 4" in sa.last_error()
    assert sa.map_post_to_sequences(m, []).shape == (0,)


def test_true_candidate_wins():
    post, cands, true_at = winner_fixture()
    for vit in (True, False):
        s = post_multi(post, cands, PEN0, vit)
        assert np.all(np.isfinite(s)) and int(np.argmax(s)) == true_at and np.sum(s == s[true_at]) == 1, (vit, s)


def test_placement_invariance():
    """the same candidates in three orders, and with duplicates: a candidate's score does not depend on where in a pack it lies"""
    post, tpath = synth.simulated_posterior(200, 9, klen=3)
    rng = np.random.default_rng(23)
    base = [_true(tpath, rng)] + [_rand(rng, n) for n in (1, 2, 3, 17, 64, 130, 255)]
    orders = [list(range(len(base))), list(range(len(base)))[::-1], [int(x) for x in rng.permutation(len(base))]]
    orders.append(orders[2] + orders[0] + [0, 0, 5])                           # duplicates
    for vit in (True, False):
        first = post_multi(post, base, PEN0, vit)
        for o in orders[1:]:
            got = post_multi(post, [base[i] for i in o], PEN0, vit)
            assert got.tobytes() == first[o].tobytes(), (vit, o)


def test_pack_split_and_oversize():
    """pack sizes 256, the default and 0 (every candidate through k_map) give the same bits; a candidate one state too long for a
    pack, and one too long for k_map's LDS home, go through k_map beside packed neighbours"""
    post, _ = synth.simulated_posterior(41, 12, klen=3)
    rng = np.random.default_rng(29)
    lens = [300, 40, 1, 2, 3, 200, 450, 60, 120, 280, 30]
    assert sum(n + 2 for n in lens) == 1508
    cands = [_rand(rng, n) for n in lens]
    for vit in (True, False):
        got = {}
        for pc in (256, 1024, -1, 0):
            sa.set_map_pack_cells(pc)
            fb, pb = sa.launch_form_counts()["map"], sa.map_pack_form_counts()
            got[pc] = post_multi(post, cands, PEN0, vit)
            fa, pa = sa.launch_form_counts()["map"], sa.map_pack_form_counts()
            assert (pa[(vit, False)] - pb[(vit, False)], fa[(vit, False, False, False)] - fb[(vit, False, False, False)]) == ((0, 1) if pc == 0 else (1, 0))
        assert got[256].tobytes() == got[1024].tobytes() == got[-1].tobytes() == got[0].tobytes(), (vit, got)
        assert got[0].tobytes() == single(post, cands, PEN0, vit).tobytes()
    sa.set_map_pack_cells(-1)
    maxc, M = sa.map_pack_max_cells(), lds_max_seq()
    assert maxc - 1 <= M
    lens = [5, maxc - 2, 40, maxc - 1, 3, M + 1, 17]            # packed alone; k_map in LDS; k_map in scratch
    cands = [_rand(rng, n) for n in lens]
    pack, _, _ = sa.map_pack_plan(lens, maxc)
    assert [int(p) < 0 for p in pack] == [False, False, False, True, False, True, False]
    for vit in (True, False):
        fb, pb = sa.launch_form_counts()["map"], sa.map_pack_form_counts()
        got = post_multi(post, cands, PEN150, vit)
        fa, pa = sa.launch_form_counts()["map"], sa.map_pack_form_counts()
        assert pa[(vit, False)] - pb[(vit, False)] == 1
        assert fa[(vit, False, False, False)] - fb[(vit, False, False, False)] == 1 and fa[(vit, False, False, True)] - fb[(vit, False, False, True)] == 1
        assert got.tobytes() == single(post, cands, PEN150, vit).tobytes(), (vit, got)


# ---------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    e.load_model("rgrgr_r94", model.synthetic_model("rgrgr_r94", seed=1))
    yield e
    e.close()


def _bases(n, rng):
    return "".join(rng.choice(list("ACGT"), n))


def _repeated(eng, sigs, lists, **kw):
    """Engine.map_to_sequence with each read repeated once per candidate: [[(score, path)] per read]"""
    flat_s = [x for x, cl in zip(sigs, lists) for _ in cl]
    flat_q = [q for cl in lists for q in cl]
    res = eng.map_to_sequence(flat_s, flat_q, **kw) if flat_s else []
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
        assert sc.dtype == np.float32 and sc.tobytes() == ws.tobytes(), (i, sc, ws)
        assert best == _best(ws), (i, best, ws)
        if path and best >= 0:
            assert np.array_equal(pth, w[best][1]), i
        else:
            assert pth is None, i


@pytest.fixture(scope="module")
def engine_reads():
    rng = np.random.default_rng(37)
    lens = [int(x) for x in rng.integers(1200, 2400, 18)]                      # two tiles, every lane index
    return [synth.medmad_normalise(synth.synthetic_signal(n, 800 + i)) for i, n in enumerate(lens)]


def test_engine_map_to_sequences(eng, engine_reads):
    rng = np.random.default_rng(39)
    sigs = engine_reads
    pens = dict(stay_pen=0.5, skip_pen=1.0, local_pen=4.0)
    shared = [_bases(n, rng) for n in (44, 300, 9, 120, 44)]
    per_read = [[_bases(int(rng.integers(6, 400)), rng) for _ in range(int(k))] for k in rng.integers(2, 7, len(sigs))]
    per_read[4] = []                                                           # K = 0
    per_read[11] = [_bases(50, rng)]                                           # K = 1
    per_read[6] = [per_read[6][0]] * 3                                         # all tie: the lowest index wins
    for lists, arg in (([shared] * len(sigs), shared), (per_read, per_read)):
        for vit in (True, False):
            before = sa.map_pack_form_counts()[(vit, True)]
            got = eng.map_to_sequences(sigs, arg, viterbi=vit, path=vit, **pens)
            assert sa.map_pack_form_counts()[(vit, True)] == before + 1        # one launch for the group
            want = _repeated(eng, sigs, lists, viterbi=vit, path=vit, **pens)
            _check_against_repeated(got, want, vit)
    assert got[4][0].shape == (0,) and got[4][1] == -1 and got[6][1] == 0
    t = eng.map_timing()
    assert t["network_ms"] > 0 and t["map_ms"] > 0
    # the route without packs: the network once, k_map per candidate
    packed = eng.map_to_sequences(sigs, per_read, viterbi=True, path=True, **pens)
    eng.debug_option("map_pack_cells", 0)
    try:
        before = sa.map_pack_form_counts()
        unpacked = eng.map_to_sequences(sigs, per_read, viterbi=True, path=True, **pens)
        assert sa.map_pack_form_counts() == before
    finally:
        eng.debug_option("map_pack_cells", -1)
    for (a, ab, ap), (b, bb, bp) in zip(unpacked, packed):
        assert a.tobytes() == b.tobytes() and ab == bb and ((ap is None and bp is None) or np.array_equal(ap, bp))


def _multi_c(eng, sigs, cand_lists, bands=None, model_name="rgrgr_r94", viterbi=1, want_path=0):
    """scrappie_hip_map_multi_batch through the C structs (state codes; bands[(i, k)] = (low, high) on candidate k of read i):
    (rc, [(scores, best)])"""
    rts, keep = sa._raw_tables(sigs)
    n = len(sigs)
    cds = (sa._MapCandidates * n)()
    for i, cl in enumerate(cand_lists):
        tgs = (sa._MapTarget * max(len(cl), 1))()
        for k, c in enumerate(cl):
            c = np.ascontiguousarray(c, dtype=np.int32)
            keep.append(c)
            tgs[k].seq = c.ctypes.data_as(C.POINTER(C.c_int))
            tgs[k].seqlen = len(c)
            if bands and (i, k) in bands:
                lo, hi = (np.ascontiguousarray(b, dtype=np.uintp) for b in bands[(i, k)])
                keep += [lo, hi]
                tgs[k].poslow = lo.ctypes.data_as(C.POINTER(C.c_size_t))
                tgs[k].poshigh = hi.ctypes.data_as(C.POINTER(C.c_size_t))
        keep.append(tgs)
        cds[i].cand, cds[i].ncand = tgs, len(cl)
    p = eng.default_params(stay_pen=0.5, skip_pen=1.0, local_pen=4.0)
    out = (sa._MapMultiResult * n)()
    rc = sa.lib().scrappie_hip_map_multi_batch(eng._h, eng._models[model_name], rts, cds, n, C.byref(p), viterbi, want_path, out)
    res = [(np.ctypeslib.as_array(r.score, shape=(r.ncand,)).copy() if r.score and r.ncand else np.zeros(0, np.float32), int(r.best))
           for r in (out[i] for i in range(n))]
    sa.lib().scrappie_hip_free_map_multi_results(out, n)
    return rc, res


def test_failures_stay_local(eng, engine_reads):
    rng = np.random.default_rng(43)
    good = [_bases(40, rng), _bases(90, rng)]
    sigs = [engine_reads[0], engine_reads[1][:5], engine_reads[2]]             # the second is below the model's minimum
    pens = dict(stay_pen=0.5, skip_pen=1.0, local_pen=4.0)
    clean = eng.map_to_sequences([sigs[0], sigs[2]], good, **pens)
    got = eng.map_to_sequences(sigs, [good[0], "ACGTNACGTACGT", "", good[1]], **pens)
    err = sa.last_error()
    assert "read 0" in err and "candidate 1" in err, err
    for (sc, best, _), (cs, cb, _) in zip((got[0], got[2]), clean):
        assert np.isnan(sc[1]) and np.isnan(sc[2]) and sc[[0, 3]].tobytes() == cs.tobytes() and best == (0, 3)[cb]
    assert np.all(np.isnan(got[1][0])) and len(got[1][0]) == 4 and got[1][1] == -1 and got[1][2] is None
    got = eng.map_to_sequences(sigs, good, **pens)
    assert "read 1" in sa.last_error() and "too short" in sa.last_error()
    assert got[0][0].tobytes() == clean[0][0].tobytes() and got[2][0].tobytes() == clean[1][0].tobytes() and np.all(np.isnan(got[1][0]))
    # a banded candidate, through the C struct: NAN there and a text, its neighbours scored
    codes = [sa.encode_bases(s, 5) for s in good]
    nb = eng.read_blocks("rgrgr_r94", len(sigs[0]))
    band = sa.diagonal_bands(4, nb, len(codes[1]))
    rc, res = _multi_c(eng, [sigs[0], sigs[2]], [[codes[0], codes[1], codes[0]], codes], bands={(0, 1): band})
    assert rc == 0 and "bands are not part of this call" in sa.last_error()
    assert np.isnan(res[0][0][1]) and res[0][0][[0, 2]].tobytes() == clean[0][0][[0, 0]].tobytes() and res[0][1] == 0
    assert res[1][0].tobytes() == clean[1][0].tobytes() and res[1][1] == clean[1][1]


def test_crf_model_is_refused(eng, engine_reads):
    eng.load_model("rnnrf_r94", model.synthetic_model("rnnrf_r94", seed=11))
    with pytest.raises(RuntimeError, match="CRF"):
        eng.map_to_sequences(engine_reads[:2], ["ACGTACGTAC"], model="rnnrf_r94")
    rc, res = _multi_c(eng, engine_reads[:2], [[np.arange(4) % 4]] * 2, model_name="rnnrf_r94")
    assert rc == -1 and "CRF" in sa.last_error() and all(len(s) == 0 and b == -1 for s, b in res)


def test_engine_map_multi_cut_by_memory(eng):
    """launch groups cut by device bytes as test_engine_map_cut_by_memory cuts them: a budget of 240 column blocks puts the reads
    of 200, 140, [300], 198 | 200, 120, 199 | 170 blocks into three groups and refuses the read of 300, which needs 319 alone;
    the others as in one uncut launch group, bit for bit"""
    lens = [1000, 700, 1500, 990, 1000, 600, 995, 850]
    rng = np.random.default_rng(51)
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 400 + i)) for i, n in enumerate(lens)]
    cands = [_bases(34, rng) for _ in range(3)]
    kw = dict(viterbi=True, path=True, stay_pen=0.5, skip_pen=1.0, local_pen=4.0)
    before = sa.map_pack_form_counts()[(True, True)]
    uncut = eng.map_to_sequences(sigs, cands, **kw)
    assert sa.map_pack_form_counts()[(True, True)] == before + 1
    assert all(np.all(np.isfinite(sc)) and best >= 0 and pth is not None for sc, best, pth in uncut)
    eng.set_max_launch_blocks(240)
    try:
        cut = eng.map_to_sequences(sigs, cands, **kw)
        err = sa.last_error()
    finally:
        eng.set_max_launch_blocks(0)
    groups = sa.map_pack_form_counts()[(True, True)] - before - 1
    print("launch groups under a budget of 240 blocks: %d" % groups)
    assert groups >= 3
    assert np.all(np.isnan(cut[2][0])) and cut[2][1] == -1 and cut[2][2] is None
    assert "read 2" in err and "too long for one launch group" in err, err
    for i, ((a, ab, ap), (b, bb, bp)) in enumerate(zip(cut, uncut)):
        if i != 2:
            assert a.tobytes() == b.tobytes() and ab == bb and np.array_equal(ap, bp), i


# ---------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------
def test_seqmappy_all_records(eng, tmp_path):
    from test_gpu_map import _fasta, _prepared
    name = "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand"
    f5 = os.path.join(READS, name + ".i16")
    own = _fasta(name)
    rng = np.random.default_rng(61)
    recs = [("decoy_a", _bases(len(own) // 2, rng)), ("own_call", own), ("decoy_b", _bases(len(own) + 40, rng))]
    fa3 = tmp_path / "three.fa"
    fa3.write_text("".join(">%s some description\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in recs))
    mfile = str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(model.synthetic_model("rgrgr_r94", seed=1), mfile)
    (scores, best, path), = eng.map_to_sequences([_prepared(f5)], [s for _, s in recs], viterbi=True, path=True)
    nb = len(path)
    r = subprocess.run([CLI, "seqmappy", "--model-file", mfile, "--all-records", str(fa3), f5], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "# %s to %s -- 3 records" % (f5, fa3) and lines[1] == "record\tname\tscore\tper_block"
    for k, (n, _) in enumerate(recs):
        assert lines[2 + k] == "%d\t%s\t%f\t%f" % (k, n, -scores[k], np.float32(-scores[k]) / np.float32(nb)), (k, lines[2 + k])
    # the record of the best: what plain seqmappy prints on a FASTA that holds only that record, under the name fasta:name
    fa1 = tmp_path / "one.fa"
    fa1.write_text(">%s\n%s\n" % recs[best])
    one = subprocess.run([CLI, "seqmappy", "--model-file", mfile, str(fa1), f5], capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr
    assert "\n".join(lines[5:]) + "\n" == one.stdout.replace(" to %s -- " % fa1, " to %s:%s -- " % (fa3, recs[best][0]), 1)
    # without the option: the first record alone, whatever follows it
    fa_first = tmp_path / "first.fa"
    fa_first.write_text(">%s\n%s\n" % recs[0])
    plain3 = subprocess.run([CLI, "seqmappy", "--model-file", mfile, str(fa3), f5], capture_output=True, text=True, timeout=600)
    plain1 = subprocess.run([CLI, "seqmappy", "--model-file", mfile, str(fa_first), f5], capture_output=True, text=True, timeout=600)
    assert plain3.returncode == 0 and plain1.returncode == 0, plain3.stderr + plain1.stderr
    assert plain3.stdout == plain1.stdout.replace(str(fa_first), str(fa3), 1)
    bad = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--all-records", str(fa3), f5], capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--all-records" in bad.stderr and bad.stdout == ""


def test_new_symbols_are_exported():
    L = sa.lib()
    for nm in ("scrappie_hip_map_multi_batch", "scrappie_hip_free_map_multi_results", "scrappie_hip_map_post_multi", "scrappie_hip_map_pack_plan",
               "scrappie_hip_map_pack_max_cells", "scrappie_hip_map_pack_form_counts"):
        assert hasattr(L, nm), nm


def test_every_pack_form_was_launched(pack_forms_at_start):
    """the last test of the module: each of the four k_map_pack instantiations (Viterbi / forward x dense / tiled) has been
    launched by the tests above"""
    now = sa.map_pack_form_counts()
    ran = {k: now[k] - pack_forms_at_start[k] for k in now}
    print("k_map_pack launches by (viterbi, tiled): %r" % sorted(ran.items()))
    assert len(ran) == 4 and all(v > 0 for v in ran.values()), ran
