"""A raw signal mapped INTO a longer reference squiggle on the GPU (k_squig_local / k_squig_local_walk, sh_squig_local.h):
Engine.match_squiggle_reference, the per-read squiggle_match_reference, Engine.mappy_reference and `scrappie mappy --inside` against
the restatement np_squiggle_local of tests/test_squiggle_local_cpu.py -- Viterbi score, first, last and padded path bit for bit, for
every stride (the restatement's score has the same bits for every stride: shown there, so one run per case stands for all) -- and,
with local_pen = 0 and an END ending, against the reference's compiled squiggle_match_viterbi.  Forward: |gpu - f64| /
(|np32 - f64| + 1e-5 |score|) under the squiggle tests' bound of 2, the float32 restatement of the same stride standing in for the
reference, which has no such function.  The sizes are those at which the windows' index arithmetic can go wrong, not workloads."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model
from test_squiggle_cpu import PENS, _case_inputs, call_squig, ref_squiggle_lib
from test_squiggle_local_cpu import END_SETS, PENS4, SCR_MUL, max_cells, need_feature, np_plan, np_squiggle_local, walk_inputs

pytestmark = pytest.mark.gpu

NSAMPLE = (1, 2, 3, 65)
NPOS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
STRIDES = (1, 7, 64, -1, 0)          # entry positions per window; the default; one window


def _kw(pens):
    return dict(rate=pens[0], back_prob=pens[1], local_pen=pens[2], skip_pen=pens[3], min_score=pens[4])


def _b(x):
    return np.float32(x).tobytes()


def _inputs(L, ns, k, seed):
    """PENS[2]'s ties on its own inputs; with back states alive a walk through positions deep inside the reference; else a simulated
    squiggle's own signal"""
    if k == 2:
        return _case_inputs(L, ns, PENS[2], seed)
    if k in (1, 3) and L >= 8:
        a = L // 3
        params, sig, _ = walk_inputs(L, a, min(L, a + ns // 2 + 2), seed)
        return params, np.resize(sig, ns).astype(np.float32)
    return _case_inputs(L, ns, PENS[0], seed)


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    return sa.squiggle_local_form_counts() if hasattr(sa, "squiggle_local_form_counts") else None


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def world():
    """per penalty set: every (npos, nsample) with its inputs and the one-window restatement (score, first, last, path, tie_free),
    computed once"""
    out = []
    for k, pens in enumerate(PENS4):
        cases = []
        for i, L in enumerate(NPOS):
            for j, ns in enumerate(NSAMPLE):
                params, sig = _inputs(L, ns, k, 7000 + 100 * k + 10 * i + j)
                info = {}
                s, first, last, path = np_squiggle_local(sig, params, *pens, info=info)
                cases.append(dict(name="L%d_s%d_set%d" % (L, ns, k), sig=sig, params=params, want=(s, first, last, path), tie_free=info["tie_free"]))
        out.append(dict(pens=pens, cases=cases))
    return out


def _check(c, got, what, path=True):
    s, first, last, pth = got
    ws, wf, wl, wp = c["want"]
    assert _b(s) == _b(ws), (what, s, ws)
    if c["tie_free"]:
        assert last == wl, (what, last, wl)
        if path:
            assert first == wf and np.array_equal(pth, wp), (what, first, wf)
    if path:
        on = pth[pth >= 0]
        assert len(pth) == len(c["sig"]) and len(on) >= 1 and first == int(on.min()) and 0 <= first < last <= len(c["params"]), what
    else:
        assert first is None and pth is None


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("stride", STRIDES)
def test_viterbi_bits(eng, world, stride, k):
    """every (npos, nsample) of one penalty set in one batched call per stride: score, first, last and path"""
    need_feature()
    w = world[k]
    eng.debug_option("squig_local_stride", stride)
    try:
        res = eng.match_squiggle_reference([c["sig"] for c in w["cases"]], [c["params"] for c in w["cases"]], viterbi=True, path=True, **_kw(w["pens"]))
        plain = eng.match_squiggle_reference([c["sig"] for c in w["cases"]], [c["params"] for c in w["cases"]], viterbi=True, path=False, **_kw(w["pens"])) if stride in (7, -1) else None
    finally:
        eng.debug_option("squig_local_stride", -1)
    free = 0
    for i, c in enumerate(w["cases"]):
        _check(c, res[i], "%s stride %d" % (c["name"], stride))
        if plain:
            _check(c, plain[i], "%s stride %d, no path" % (c["name"], stride), path=False)
        free += c["tie_free"]
    assert len(res) == 40 and (free >= 20 or k == 2)


def test_homes_at_the_cell_limit(eng):
    """max_cells + 300 positions, 40 samples: the default stride's windows live in LDS, one window lives in device scratch; the same
    bits, both homes launched"""
    need_feature()
    M = max_cells()
    assert sa.squiggle_local_max_cells() == M
    L, ns = M + 300, 40
    params, sig, walk = walk_inputs(L, M - 20, M + 10, 77)
    sig = np.resize(sig, ns).astype(np.float32)
    pens = PENS4[1]
    info = {}
    want = np_squiggle_local(sig, params, *pens, info=info)
    plan = sa.squiggle_local_plan(L, ns, -1)
    assert len(plan["first"]) == 2 and not plan["home"].any() and int(plan["ncell"][0]) == M - 1      # (window 0 keeps no cell to its left)
    assert sa.squiggle_local_plan(L, ns, 0)["home"].tolist() == [1]
    got = {}
    for stride in (-1, 0, M - 77, M - 78):          # windows of exactly M and M + 1 cells too
        eng.debug_option("squig_local_stride", stride)
        try:
            b0 = sa.squiggle_local_form_counts()
            got[stride] = eng.match_squiggle_reference([sig], params, viterbi=True, path=True, **_kw(pens))[0]
            fwd = eng.match_squiggle_reference([sig], params, viterbi=False, **_kw(pens))[0]
            b1 = sa.squiggle_local_form_counts()
        finally:
            eng.debug_option("squig_local_stride", -1)
        homes = set(int(h) for h in sa.squiggle_local_plan(L, ns, stride)["home"])
        for scratch in (False, True):          # (the first pass launches every home of the plan, the second the best window's)
            assert (b1[(True, scratch)] > b0[(True, scratch)]) == (int(scratch) in homes), (stride, scratch, b0, b1)
            assert b1[(False, scratch)] - b0[(False, scratch)] == (1 if int(scratch) in homes else 0), (stride, scratch)
        assert np.isfinite(fwd[0]) and fwd[0] >= got[stride][0]
        c = dict(sig=sig, params=params, want=want, tie_free=info["tie_free"])
        _check(c, got[stride], "stride %d" % stride)
    assert int(sa.squiggle_local_plan(L, ns, M - 78)["ncell"][0]) == M and int(sa.squiggle_local_plan(L, ns, M - 77)["ncell"][0]) == M + 1
    assert want[1] >= M - 22                                 # it lies across the first window's last cells
    assert len({_b(g[0]) for g in got.values()}) == 1
    if info["tie_free"]:
        assert len({(g[1], g[2], g[3].tobytes()) for g in got.values()}) == 1


def test_scratch_read_before_lds_read_in_one_call(eng):
    """two reads into one reference of three whole scratch windows, in this order: one of so many samples that the default stride
    puts its windows in device scratch, one of 40 whose windows live in LDS.  The second pass then runs the reads in another order
    than the call's (LDS home first): score, first, last and path of each as of the read called alone, bit for bit"""
    need_feature()
    M = max_cells()
    ns_scr, ns_lds = M // 4 + 2, 40
    L = 3 * SCR_MUL * ns_scr
    params, long_sig, _ = walk_inputs(L, M + 50, M + 50 + ns_scr // 2 + 2, 91)
    same, short_sig, _ = walk_inputs(L, 2 * M + 10, 2 * M + 40, 91)
    assert np.array_equal(params, same)
    reads = [np.resize(long_sig, ns_scr).astype(np.float32), np.resize(short_sig, ns_lds).astype(np.float32)]
    scr, lds = sa.squiggle_local_plan(L, ns_scr, -1), sa.squiggle_local_plan(L, ns_lds, -1)
    assert len(scr["home"]) >= 3 and scr["home"].all() and len(lds["home"]) >= 3 and not lds["home"].any()
    kw = _kw(PENS4[1])
    b0 = sa.squiggle_local_form_counts()
    together = eng.match_squiggle_reference(reads, params, viterbi=True, path=True, **kw)
    b1 = sa.squiggle_local_form_counts()
    assert b1[(True, False)] - b0[(True, False)] == 2 and b1[(True, True)] - b0[(True, True)] == 2, (b0, b1)      # both homes in both passes
    alone = [eng.match_squiggle_reference([r], params, viterbi=True, path=True, **kw)[0] for r in reads]
    for i, (got, want) in enumerate(zip(together, alone)):
        assert np.isfinite(want[0]) and _b(got[0]) == _b(want[0]) and got[1:3] == want[1:3] and np.array_equal(got[3], want[3]), i
        assert len(got[3]) == len(reads[i]) and got[1] == int(got[3][got[3] >= 0].min()), i


def test_without_local_penalty_against_the_compiled_reference(eng, world):
    """local_pen = 0, two samples at 50.0 behind every signal: the path ends in END and the score is the bits of
    oracle/_ref/libref_decode.so's squiggle_match_viterbi; the path too wherever no tie was met"""
    need_feature()
    R = ref_squiggle_lib()
    assert R is not None, "oracle/_ref/libref_decode.so is required (build() makes it and it travels with the tree)"
    same = 0
    for si, pens in enumerate(END_SETS):
        cases = world[si]["cases"]
        sigs = [np.concatenate((c["sig"], np.float32([50.0, 50.0]))).astype(np.float32) for c in cases]
        infos = [dict() for _ in cases]
        wants = [np_squiggle_local(x, c["params"], *pens, info=i) for c, x, i in zip(cases, sigs, infos)]
        for stride in (-1, 7):
            eng.debug_option("squig_local_stride", stride)
            try:
                res = eng.match_squiggle_reference(sigs, [c["params"] for c in cases], viterbi=True, path=True, **_kw(pens))
            finally:
                eng.debug_option("squig_local_stride", -1)
            for c, x, i, w, (s, first, last, pth) in zip(cases, sigs, infos, wants, res):
                want_s, want_p = call_squig(R, x, 0, len(x), c["params"], pens, True)
                assert i["ends_in_end"] and want_p[-1] == -1 and np.any(want_p >= 0) and pth[-1] == -1, c["name"]
                assert _b(s) == want_s.tobytes() == _b(w[0]), (c["name"], pens, stride, s, want_s)
                if i["tie_free"]:
                    assert np.array_equal(pth, want_p) and (first, last) == w[1:3], (c["name"], pens, stride)
                    same += 1
    assert same >= 40


@pytest.mark.parametrize("k", range(4))
def test_forward(eng, world, k):
    """|gpu - f64| / (|np32 - f64| + 1e-5 |score|) < 2, the float32 restatement of the same stride for the reference"""
    need_feature()
    w = world[k]
    worst = 0.0
    for stride in (7, -1, 0):
        cases = [c for c in w["cases"] if stride != 7 or len(c["params"]) <= 257 or len(c["sig"]) <= 3]
        eng.debug_option("squig_local_stride", stride)
        try:
            res = eng.match_squiggle_reference([c["sig"] for c in cases], [c["params"] for c in cases], viterbi=False, **_kw(w["pens"]))
        finally:
            eng.debug_option("squig_local_stride", -1)
        for c, (s, first, last, pth) in zip(cases, res):
            assert first is None and last is None and pth is None
            np32 = float(np_squiggle_local(c["sig"], c["params"], *w["pens"], stride=stride, viterbi=False)[0])
            f64 = float(np_squiggle_local(c["sig"], c["params"], *w["pens"], stride=stride, viterbi=False, dtype=np.float64)[0])
            ratio = abs(float(s) - f64) / (abs(np32 - f64) + 1e-5 * abs(f64))
            print("forward %s stride %d: gpu %r np32 %r f64 %r ratio %.3f" % (c["name"], stride, float(s), np32, f64, ratio))
            worst = max(worst, ratio)
            assert ratio < 2, (c["name"], stride, s, np32, f64)
            assert float(s) >= float(c["want"][0]) - 1e-4 * abs(f64)          # the sum holds the best path
    print("local forward, set %d: worst |gpu - f64| / (|np32 - f64| + 1e-5 |score|) = %.3f" % (k, worst))


def test_window_inside_a_padded_read(eng, world):
    need_feature()
    c = world[1]["cases"][-1]
    pad = np.random.RandomState(5).normal(0.0, 1.0, size=200).astype(np.float32)
    pad[70:135] = c["sig"]
    rt = sa.RawTable(pad, start=70, end=135)
    s, first, last, pth = eng.match_squiggle_reference([rt], c["params"], viterbi=True, path=True, **_kw(world[1]["pens"]))[0]
    assert _b(s) == _b(c["want"][0]) and len(pth) == 200 and np.all(pth[:70] == -1) and np.all(pth[135:] == -1)
    if c["tie_free"]:
        assert (first, last) == c["want"][1:3] and np.array_equal(pth[70:135], c["want"][3])
    s2, f2, l2, p2 = sa.squiggle_match_reference(rt, c["params"], *world[1]["pens"], viterbi=True, path=True)
    assert _b(s2) == _b(s) and (f2, l2) == (first, last) and np.array_equal(p2, pth)


def test_shared_and_per_read_references_and_launches(eng, world):
    """one reference object for several reads beside per-read ones in one call; a small budget that forces several launches, and a
    read that fits none"""
    need_feature()
    w = world[1]
    kw = _kw(w["pens"])
    big = [c for c in w["cases"] if len(c["params"]) == 1000]
    A, B = big[3]["params"], w["cases"][20]["params"]
    reads = [c["sig"] for c in big] + [w["cases"][20]["sig"], big[3]["sig"]]
    refs = [A, A, A, A, B, A]
    key = lambda res: [(_b(s), f, l, p.tobytes()) for s, f, l, p in res]
    together = eng.match_squiggle_reference(reads, refs, viterbi=True, path=True, **kw)
    alone = [eng.match_squiggle_reference([r], [q], viterbi=True, path=True, **kw)[0] for r, q in zip(reads, refs)]
    shared = eng.match_squiggle_reference(reads[:4], A, viterbi=True, path=True, **kw)
    assert key(together) == key(alone) and key(shared) == key(together[:4])
    _check(big[3], together[3], "shared")
    _check(big[3], together[5], "shared, again")
    long_read = np.ascontiguousarray(np.resize(big[3]["sig"], 4000))
    eng.debug_option("squiggle_budget_kb", 160)
    try:
        b0 = sa.squiggle_local_form_counts()
        res = eng.match_squiggle_reference(reads[:3] + [long_read] + reads[3:], refs[:3] + [A] + refs[3:], viterbi=True, path=True, **kw)
        err = sa.last_error()
        b1 = sa.squiggle_local_form_counts()
    finally:
        eng.debug_option("squiggle_budget_kb", 0)
    assert sum(b1.values()) - sum(b0.values()) >= 4, (b0, b1)          # two passes each of at least two launches
    assert np.isnan(res[3][0]) and res[3][1:] == (None, None, None) and "read 3" in err and "more than one launch may take" in err, err
    assert key(res[:3] + res[4:]) == key(together)


def test_error_locality(eng, world):
    need_feature()
    w = world[0]
    kw = _kw(w["pens"])
    cs = w["cases"][12:20]
    good = eng.match_squiggle_reference([c["sig"] for c in cs], [c["params"] for c in cs], viterbi=True, path=True, **kw)
    key = lambda res: [(_b(s), f, l, p.tobytes()) for s, f, l, p in res]
    reads = [c["sig"] for c in cs]
    refs = [c["params"] for c in cs]
    reads.insert(2, sa.RawTable(cs[3]["sig"], start=1, end=1))
    refs.insert(2, cs[3]["params"])
    reads.insert(5, cs[4]["sig"])
    refs.insert(5, np.zeros((0, 3), dtype=np.float32))
    res = eng.match_squiggle_reference(reads, refs, viterbi=True, path=True, **kw)
    assert "read 2" in sa.last_error() and "empty" in sa.last_error()
    for i in (2, 5):
        assert np.isnan(res[i][0]) and res[i][1:] == (None, None, None)
    assert key([r for i, r in enumerate(res) if i not in (2, 5)]) == key(good)
    assert eng.match_squiggle_reference([], refs[0]) == []
    eng.debug_option("fail_run", 1)
    with pytest.raises(RuntimeError, match="injected failure"):
        eng.match_squiggle_reference([c["sig"] for c in cs], [c["params"] for c in cs], viterbi=True, path=True, **kw)
    again = eng.match_squiggle_reference([c["sig"] for c in cs], [c["params"] for c in cs], viterbi=True, path=True, **kw)
    assert key(again) == key(good)


def test_per_read_surface(world):
    """squiggle_match_reference on the process-default engine, under its own stride option"""
    need_feature()
    w = world[3]
    try:
        for stride in (-1, 7, 0):
            sa.set_squiggle_local_stride(stride)
            for i in (11, 27, 39):
                c = w["cases"][i]
                _check(c, sa.squiggle_match_reference(sa.RawTable(c["sig"]), c["params"], *w["pens"], viterbi=True, path=True), c["name"])
                s, first, last, pth = sa.squiggle_match_reference(sa.RawTable(c["sig"]), c["params"], *w["pens"], viterbi=True)
                assert _b(s) == _b(c["want"][0]) and first is None and pth is None and (last == c["want"][2] or not c["tie_free"])
    finally:
        sa.set_squiggle_local_stride(-1)
    c = w["cases"][39]
    f = sa.squiggle_match_reference(sa.RawTable(c["sig"]), c["params"], *w["pens"], viterbi=False)
    assert np.isfinite(f[0]) and f[1:] == (None, None, None)


# ---------------------------------------------------------------------------
# Engine.mappy_reference and scrappie mappy --inside
# ---------------------------------------------------------------------------
READ = "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand"


def test_mappy_reference_and_inside(fast5_dir, tmp_path):
    """a synthetic squiggle model in a file, a bundled read trimmed and scaled, and a reference cut from its sequence: the Engine
    call predicts each distinct sequence once; the command line prints the same mapping with `positions first..last` in its header"""
    need_feature()
    from test_sqnet_cpu import CLI, ROOT, weights
    name = "squiggle_r94"
    mf = str(tmp_path / (name + ".scrm"))
    model.save_model(weights(name), mf)
    f5 = os.path.join(fast5_dir, READ + ".fast5")
    seq = "".join(l.strip() for l in open(os.path.join(ROOT, "tests", "golden", "reads", READ + ".fa")).read().splitlines()[1:])
    ref_seq, other = seq[:600], seq[100:400]
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as fh:
        fh.write(">ref\n%s\n" % ref_seq)
    L = sa.lib()
    rt = L.scrappie_hip_read_raw(os.fsencode(f5), True)
    raw = np.ctypeslib.as_array(rt.raw, shape=(rt.n,)).copy()
    sa._libc.free(C.cast(rt.raw, C.c_void_p))
    trimmed = sa.RawTable(raw).trim().scale()
    e = sa.Engine(0)
    try:
        e.load_model(name, mf)
        n0 = int(L.scrappie_hip_sqnet_launch_count())
        res = e.mappy_reference([trimmed, trimmed, trimmed], [ref_seq, other, ref_seq], model=name)
        assert int(L.scrappie_hip_sqnet_launch_count()) == n0 + 1
        one = e.mappy_reference([trimmed], ref_seq, model=name)[0]
        sq = e.predict_squiggle([ref_seq], model=name)[0]
        direct = e.match_squiggle_reference([trimmed], sq, viterbi=True, path=True)[0]
        bad = e.mappy_reference([trimmed, trimmed], [ref_seq, "ACG"], model=name)
    finally:
        e.close()
    key = lambda r: (_b(r[0]), r[1], r[2], r[3].tobytes())
    assert key(res[0]) == key(res[2]) == key(one) == key(direct) == key(bad[0]) and key(res[1]) != key(res[0])
    assert np.isnan(bad[1][0]) and bad[1][1:] == (None, None, None)
    s, first, last, pth = one
    assert 0 <= first < last <= len(ref_seq) and len(pth) == len(raw)
    r = subprocess.run([CLI, "mappy", "--inside", "--model-file", mf, fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "# %s to %s  (score = %f, positions %d..%d)" % (f5, fa, s, first, last), lines[0]
    assert len(lines) == 2 + len(raw)
    got = np.array([int(l.split("\t")[2]) for l in lines[2:]], dtype=np.int32)
    assert np.array_equal(got, pth)
    for l, p in zip(lines[2:], pth):
        if p >= 0:
            assert l.split("\t")[3] == ref_seq[p]
    r = subprocess.run([CLI, "mappy", "--inside", "--band", "5", "--model-file", mf, fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--inside" in r.stderr


def test_every_form_was_launched(forms_at_start):
    need_feature()
    now = sa.squiggle_local_form_counts()
    for form in now:
        assert now[form] > forms_at_start[form], form
