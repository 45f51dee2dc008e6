"""One signal against many candidate squiggles on the GPU (k_squig_pack, sh_squig_pack.h): Engine.match_squiggles and
the per-read squiggle_match_many against the reference's compiled decode.c (oracle/_ref/libref_decode.so) and against
Engine.match_squiggle pair by pair.  Viterbi scores are bit-identical for every pack setting and the best candidate's
path is match_squiggle's; forward within 2x the reference's own error + 1e-5 |score| (_forward_ok of
tests/test_gpu_squiggle.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model
from test_squiggle_cpu import PENS, _case_inputs, call_squig, lds_threshold, np_squiggle_match, ref_squiggle_lib

pytestmark = pytest.mark.gpu

# npos 1, 2 and 3 beside each other and beside long candidates; at the largest pack setting 257 starts at cell 6 (mid-wave) and
# crosses the lane edges and the chunk edge at 256; at the default 64 starts at cell 66 and crosses cell 128
NPOS = (2, 1, 3, 257, 1, 63, 2, 64, 3, 65, 4, 255, 256)
NSAMPLE = (1, 2, 3, 65, 400)


def _kw(pens):
    return dict(rate=pens[0], back_prob=pens[1], local_pen=pens[2], skip_pen=pens[3], min_score=pens[4])


def _b(x):
    return np.float32(x).tobytes()


@pytest.fixture(scope="module")
def ref():
    R = ref_squiggle_lib()
    assert R is not None, "oracle/_ref/libref_decode.so is required (build() makes it and it travels with the tree)"
    return R


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    return sa.squiggle_pack_form_counts()


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(ref):
    """per penalty set: the candidates, the reads, and the reference's Viterbi (score, path) of every pair, computed once"""
    out = []
    for s, pens in enumerate(PENS):
        cands = [_case_inputs(npos, 400, pens, 300 + 17 * s + k)[0] for k, npos in enumerate(NPOS)]
        sig = _case_inputs(65, 400, pens, 300 + 17 * s + 9)[1]          # the signal simulated from the candidate of 65 positions
        reads = [np.ascontiguousarray(sig[:ns]) for ns in NSAMPLE]
        want = [[call_squig(ref, r, 0, len(r), c, pens, True) for c in cands] for r in reads]
        out.append(dict(pens=pens, cands=cands, reads=reads, want=want))
    return out


def test_arrangement_reaches_the_edges():
    mx = sa.squiggle_pack_max_cells()
    pack, cell, _ = sa.squiggle_pack_plan(NPOS, mx)
    k = NPOS.index(257)
    assert pack[k] == 0 and cell[k] % 64 not in (0,) and cell[k] < 256 < cell[k] + 257          # mid-wave, over lane edges and the chunk edge
    pack, cell, _ = sa.squiggle_pack_plan(NPOS, 256)
    k = NPOS.index(64)
    assert 0 < cell[k] % 64 and cell[k] // 64 != (cell[k] + 63) // 64
    for a, b in ((0, 1), (1, 2), (2, 3)):                    # 2, 1, 3 and 257 in a row
        assert NPOS[a] <= 3 and (NPOS[b] <= 3 or NPOS[b] == 257)


@pytest.mark.parametrize("s", [0, 1, 2])
def test_viterbi_bits(eng, world, s):
    """every (read, candidate): the score is the compiled reference's and Engine.match_squiggle's in bits; the best candidate and
    its path are match_squiggle's"""
    w = world[s]
    before = sa.squiggle_pack_form_counts()
    res = eng.match_squiggles(w["reads"], w["cands"], viterbi=True, path=True, **_kw(w["pens"]))
    assert sa.squiggle_pack_form_counts()[True] == before[True] + 1           # reads of five lengths, all their packs: one launch
    pr, pc = zip(*[(r, c) for r in w["reads"] for c in w["cands"]])
    single = eng.match_squiggle(list(pr), list(pc), viterbi=True, path=True, **_kw(w["pens"]))
    assert len(res) == len(NSAMPLE)
    for i, (sc, best, pth) in enumerate(res):
        assert sc.dtype == np.float32 and len(sc) == len(NPOS)
        for k in range(len(NPOS)):
            assert sc[k].tobytes() == w["want"][i][k][0].tobytes(), (s, NSAMPLE[i], NPOS[k], sc[k], w["want"][i][k][0])
            assert sc[k].tobytes() == _b(single[i * len(NPOS) + k][0]), (s, NSAMPLE[i], NPOS[k])
        assert best == int(np.argmax(sc)) and sc[best] == sc.max()          # (argmax: the lowest index on a tie)
        assert np.array_equal(pth, single[i * len(NPOS) + best][1]) and np.array_equal(pth, w["want"][i][best][1]), (s, NSAMPLE[i], best)


def test_pack_settings_give_same_bytes(eng, world):
    mx = sa.squiggle_pack_max_cells()
    try:
        for w in world:
            first = None
            for cells, lone in ((0, 0), (64, 0), (256, 0), (-1, 0), (mx, 0), (64, 1), (256, 1), (mx, 1)):
                eng.debug_option("squig_pack_cells", cells)
                eng.debug_option("squig_pack_lone", lone)          # 1: a candidate alone in its pack runs packed too
                b0, q0 = sa.squiggle_pack_form_counts(), sa.launch_form_counts()["squig"]
                res = eng.match_squiggles(w["reads"], w["cands"], viterbi=True, path=True, **_kw(w["pens"]))
                b1, q1 = sa.squiggle_pack_form_counts(), sa.launch_form_counts()["squig"]
                assert b1[False] == b0[False]
                if cells == 0:
                    assert b1[True] == b0[True] and q1[(True, False)] == q0[(True, False)] + 2       # the candidates, then the paths
                else:
                    assert b1[True] == b0[True] + 1
                got = [(sc.tobytes(), best, pth.tobytes()) for sc, best, pth in res]
                if first is None:
                    first = got
                assert got == first, (cells, lone)
            for i, (sc, best, pth) in enumerate(res):
                assert sc.tobytes() == b"".join(w["want"][i][k][0].tobytes() for k in range(len(NPOS)))
    finally:
        eng.debug_option("squig_pack_cells", -1)
        eng.debug_option("squig_pack_lone", 0)


def test_pack_limits(eng, ref):
    """a pack of exactly max_cells cells (three candidates; with squig_pack_lone also one candidate) runs packed, max_cells + 1 positions take
    k_squig's LDS home and lds_threshold() + 1 its scratch home, in one call with short candidates: the bytes of each pair alone"""
    mx, T = sa.squiggle_pack_max_cells(), lds_threshold()
    npos = [5, mx, 2, mx + 1, T + 1, mx - 9, 7, 1]
    pack, cell, npack = sa.squiggle_pack_plan(npos, mx)
    assert list(pack) == [0, 1, 2, -1, -1, 2, 2, 3] and npack == 4 and cell[6] + 7 == mx
    pens = PENS[1]
    cands = [_case_inputs(n, 40, pens, 900 + k)[0] for k, n in enumerate(npos)]
    sig = np.ascontiguousarray(_case_inputs(mx, 41, pens, 901)[1][:41])
    single = eng.match_squiggle([sig] * len(npos), cands, viterbi=True, path=True, **_kw(pens))
    eng.debug_option("squig_pack_cells", mx)
    try:
        for lone in (0, 1):
            eng.debug_option("squig_pack_lone", lone)
            b0, q0 = sa.squiggle_pack_form_counts(), sa.launch_form_counts()["squig"]
            (sc, best, pth), = eng.match_squiggles([sig], cands, viterbi=True, path=True, **_kw(pens))
            b1, q1 = sa.squiggle_pack_form_counts(), sa.launch_form_counts()["squig"]
            assert b1[True] == b0[True] + 1
            assert q1[(True, True)] == q0[(True, True)] + 1 + (npos[best] > T)          # T + 1 positions: the scratch home
            assert q1[(True, False)] == q0[(True, False)] + 1 + (npos[best] <= T)       # max_cells + 1: the LDS home; the best one's path
            for k in range(len(npos)):
                assert sc[k].tobytes() == _b(single[k][0]) == call_squig(ref, sig, 0, len(sig), cands[k], pens, True)[0].tobytes(), (lone, npos[k])
            assert np.array_equal(pth, single[best][1])
    finally:
        eng.debug_option("squig_pack_cells", -1)
        eng.debug_option("squig_pack_lone", 0)


def test_forward(eng, ref, world):
    worst = 0.0
    for w in world:
        reads = [w["reads"][i] for i in (2, 3, 4)]
        res = eng.match_squiggles(reads, w["cands"], viterbi=False, **_kw(w["pens"]))
        for r, (sc, best, pth) in zip(reads, res):
            assert pth is None
            for k, c in enumerate(w["cands"]):
                rf = float(call_squig(ref, r, 0, len(r), c, w["pens"], False)[0])
                f64 = float(np_squiggle_match(r, c, *w["pens"], viterbi=False, dtype=np.float64)[0])
                eg, er = abs(float(sc[k]) - f64), abs(rf - f64)
                print("forward ns %d npos %d: gpu %r ref %r f64 %r" % (len(r), len(c), float(sc[k]), rf, f64))
                assert eg <= 2 * er + 1e-5 * abs(f64), (len(r), len(c), sc[k], rf, f64)
                worst = max(worst, eg / (er + 1e-5 * abs(f64) + 1e-30))
            assert best == int(np.argmax(sc))
    print("forward, packs: worst |gpu - f64| / (|ref - f64| + 1e-5 |score|) = %.3f" % worst)


def test_shared_and_per_read_sets(eng, world):
    w = world[1]
    kw = _kw(w["pens"])
    shared = eng.match_squiggles(w["reads"], w["cands"], viterbi=True, path=True, **kw)
    per = eng.match_squiggles(w["reads"], [list(w["cands"]) for _ in w["reads"]], viterbi=True, path=True, **kw)
    alone = [eng.match_squiggles([r], w["cands"], viterbi=True, path=True, **kw)[0] for r in w["reads"]]
    key = lambda res: [(sc.tobytes(), best, pth.tobytes()) for sc, best, pth in res]
    assert key(shared) == key(per) == key(alone)
    # several launches, and one read that fits none (its second pass alone is over the budget)
    long_read = np.ascontiguousarray(np.tile(w["reads"][4], 40))
    reads = w["reads"][:3] + [long_read] + w["reads"][3:]
    eng.debug_option("squiggle_budget_kb", 160)
    try:
        b0 = sa.squiggle_pack_form_counts()
        res = eng.match_squiggles(reads, w["cands"], viterbi=True, path=True, **kw)
        err = sa.last_error()
        b1 = sa.squiggle_pack_form_counts()
    finally:
        eng.debug_option("squiggle_budget_kb", 0)
    assert b1[True] - b0[True] >= 2, (b0, b1)
    assert np.all(np.isnan(res[3][0])) and res[3][1] == -1 and res[3][2] is None and "read 3" in err and "more than one launch may take" in err, err
    assert key(res[:3] + res[4:]) == key(shared)


def test_error_locality(eng, world):
    w = world[0]
    kw = _kw(w["pens"])
    good = eng.match_squiggles(w["reads"], w["cands"], viterbi=True, path=True, **kw)
    cands = list(w["cands"])
    cands.insert(4, np.zeros((0, 3), dtype=np.float32))
    cands.insert(8, np.ascontiguousarray(w["cands"][5][:, :2]))
    keep = [k for k in range(len(cands)) if k not in (4, 8)]
    res = eng.match_squiggles(w["reads"], cands, viterbi=True, path=True, **kw)
    assert "candidate 4" in sa.last_error()
    for (sc, best, pth), (gs, gb, gp) in zip(res, good):
        assert np.isnan(sc[4]) and np.isnan(sc[8])
        assert sc[keep].tobytes() == gs.tobytes() and keep[gb] == best and np.array_equal(pth, gp)
    # a read that cannot be matched (an empty window) between good ones; a read without candidates
    bad = sa.RawTable(w["reads"][3], start=5, end=5)
    res = eng.match_squiggles([w["reads"][0], bad, w["reads"][4]], [w["cands"], w["cands"], []], viterbi=True, path=True, **kw)
    assert "read 1" in sa.last_error() and "empty" in sa.last_error()
    assert res[0][0].tobytes() == good[0][0].tobytes() and np.array_equal(res[0][2], good[0][2])
    assert len(res[1][0]) == len(NPOS) and np.all(np.isnan(res[1][0])) and res[1][1] == -1 and res[1][2] is None
    assert len(res[2][0]) == 0 and res[2][1] == -1 and res[2][2] is None
    assert eng.match_squiggles([], w["cands"]) == []
    # a failed launch fails the call with its text; the next call is clean
    eng.debug_option("fail_run", 1)
    with pytest.raises(RuntimeError, match="injected failure"):
        eng.match_squiggles(w["reads"], w["cands"], viterbi=True, path=True, **kw)
    again = eng.match_squiggles(w["reads"], w["cands"], viterbi=True, path=True, **kw)
    assert [(a.tobytes(), b, c.tobytes()) for a, b, c in again] == [(a.tobytes(), b, c.tobytes()) for a, b, c in good]


def test_per_read_surface(world):
    """squiggle_match_many on the process-default engine: the same bytes, Viterbi, under its own pack settings"""
    w = world[1]
    try:
        for cells in (-1, 0):
            sa.set_squiggle_pack_cells(cells)
            for i in (1, 3):
                sc = sa.squiggle_match_many(sa.RawTable(w["reads"][i]), w["cands"], *w["pens"], viterbi=True)
                assert sc.dtype == np.float32
                assert sc.tobytes() == b"".join(w["want"][i][k][0].tobytes() for k in range(len(NPOS)))
    finally:
        sa.set_squiggle_pack_cells(-1)
    fw = sa.squiggle_match_many(sa.RawTable(w["reads"][3]), w["cands"], *w["pens"], viterbi=False)
    assert np.all(np.isfinite(fw))


# ---------------------------------------------------------------------------
# Engine.mappy_multi and scrappie mappy --all-records
# ---------------------------------------------------------------------------
READ = "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand"


@pytest.fixture(scope="module")
def mappy_setup(fast5_dir, tmp_path_factory):
    """a synthetic squiggle model in a file (as tests/test_gpu_squiggle_band.py makes it), a bundled read trimmed and scaled, and a
    fasta of five records cut from its sequence: two short slices, one too long for a pack, a third short one and the first slice
    again under another name"""
    from test_sqnet_cpu import CLI, ROOT, weights
    name = "squiggle_r94"
    d = tmp_path_factory.mktemp("pack_mappy")
    mf = str(d / (name + ".scrm"))
    model.save_model(weights(name), mf)
    f5 = os.path.join(fast5_dir, READ + ".fast5")
    seq = "".join(l.strip() for l in open(os.path.join(ROOT, "tests", "golden", "reads", READ + ".fa")).read().splitlines()[1:])
    mx = sa.squiggle_pack_max_cells()
    assert len(seq) > mx + 60 and mx > 320
    recs = [("first", seq[50:200]), ("head", seq[:90]), ("long", seq[:mx + 60]), ("middle", seq[100:300]), ("first_again", seq[50:200])]
    fa = str(d / "records.fa")
    with open(fa, "w") as fh:
        for nm, sq in recs:
            fh.write(">%s\n%s\n" % (nm, sq))
    L = sa.lib()
    rt = L.scrappie_hip_read_raw(os.fsencode(f5), True)
    raw = np.ctypeslib.as_array(rt.raw, shape=(rt.n,)).copy()
    sa._libc.free(C.cast(rt.raw, C.c_void_p))
    trimmed = sa.RawTable(raw).trim().scale()

    def run(fasta, *opts, ok=True):
        r = subprocess.run([CLI, "mappy", "--model-file", mf] + list(opts) + [fasta, f5], capture_output=True, text=True, timeout=120)
        assert (r.returncode == 0) == ok, r.stderr
        return r.stdout if ok else r.stderr
    return dict(name=name, mf=mf, fa=fa, f5=f5, recs=recs, run=run, trimmed=trimmed, dir=d, nraw=len(raw))


def test_mappy_multi_and_all_records(mappy_setup):
    m = mappy_setup
    seqs = [s for _, s in m["recs"]]
    e = sa.Engine(0)
    try:
        e.load_model(m["name"], m["mf"])
        single = e.mappy([m["trimmed"]] * len(seqs), seqs, model=m["name"])
        n0 = int(sa.lib().scrappie_hip_sqnet_launch_count())
        b0 = sa.squiggle_pack_form_counts()
        (sc, best, pth), (sc2, best2, pth2) = e.mappy_multi([m["trimmed"], m["trimmed"]], [seqs, seqs[:2] + seqs[3:]], model=m["name"])
        assert int(sa.lib().scrappie_hip_sqnet_launch_count()) == n0 + 1          # the distinct sequences of both reads: one prediction
        assert sa.squiggle_pack_form_counts()[True] == b0[True] + 1
        shared = e.mappy_multi([m["trimmed"]], seqs, model=m["name"])[0]
    finally:
        e.close()
    for k in range(len(seqs)):
        assert sc[k].tobytes() == _b(single[k][0]), m["recs"][k][0]
    assert sc[0].tobytes() == sc[4].tobytes() and best == int(np.argmax(sc)) and np.array_equal(pth, single[best][1])
    assert sc2.tobytes() == sc[[0, 1, 3, 4]].tobytes() and np.array_equal(pth2, single[[0, 1, 3, 4][best2]][1])
    assert shared[0].tobytes() == sc.tobytes() and shared[1] == best and np.array_equal(shared[2], pth)
    # the command line: the table, then the best record as plain mappy prints it from a fasta of that record alone
    lines = m["run"](m["fa"], "--all-records").splitlines()
    assert lines[0] == "record\tname\tscore\tper_sample"
    ns = m["trimmed"].end - m["trimmed"].start
    for k, (nm, _) in enumerate(m["recs"]):
        assert lines[1 + k] == "%d\t%s\t%f\t%f" % (k, nm, sc[k], np.float32(sc[k]) / np.float32(ns)), lines[1 + k]
    alone = str(m["dir"] / "alone.fa")
    with open(alone, "w") as fh:
        fh.write(">%s\n%s\n" % m["recs"][best])
    want = m["run"](alone).splitlines()
    got = lines[1 + len(seqs):]
    assert got[0] == want[0].replace(alone, m["fa"]) == "# %s to %s  (score = %f)" % (m["f5"], m["fa"], sc[best])
    assert got[1:] == want[1:] and len(got) == 2 + m["nraw"]
    assert "--band" in m["run"](m["fa"], "--all-records", "--band", "5", ok=False)


def test_every_pack_form_was_launched(forms_at_start):
    now = sa.squiggle_pack_form_counts()
    assert now[True] > forms_at_start[True] and now[False] > forms_at_start[False]
