"""Squiggle matching on the GPU (sh_squig.h): the per-read squiggle_match_viterbi / _forward and the batched
Engine.match_squiggle against the reference's compiled decode.c (oracle/_ref/libref_decode.so) and the numpy restatement
of tests/test_squiggle_cpu.py.  Viterbi scores and padded paths must be bit-identical; forward within 2x the reference's
own error + 1e-5 |score| (the criterion of tests/test_gpu_map.py)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import synth
from test_squiggle_cpu import (PENS, call_squig, lds_threshold, np_squiggle_match, ref_squiggle_lib, squig_cases,
                               squig_scratch_cases)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    R = ref_squiggle_lib()
    assert R is not None, "oracle/_ref/libref_decode.so is required (build() makes it and it travels with the tree)"
    return R


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """k_squig launches per form before this module's first test (test_every_squig_form_was_launched)"""
    return sa.launch_form_counts()["squig"]


def _with_references(ref, raw):
    out = []
    for name, sig, start, end, params, pens in raw:
        c = dict(name=name, sig=sig, start=start, end=end, params=params, pens=pens)
        c["ref_v"] = call_squig(ref, sig, start, end, params, pens, True)
        c["ref_f"] = call_squig(ref, sig, start, end, params, pens, False)[0]
        c["np_v"] = np_squiggle_match(sig[start:end], params, *pens, viterbi=True)
        c["f64"] = float(np_squiggle_match(sig[start:end], params, *pens, viterbi=False, dtype=np.float64)[0])
        out.append(c)
    return out


@pytest.fixture(scope="module")
def cases(ref):
    """every case with what the reference and the restatement give for it, computed once"""
    return _with_references(ref, squig_cases(lds_threshold()))


@pytest.fixture(scope="module")
def scratch_cases(ref):
    """squig_scratch_cases (every one in the scratch home), likewise"""
    return _with_references(ref, squig_scratch_cases(lds_threshold()))


def _forward_ok(got, want_ref, exact, name):
    """|gpu - f64| <= 2 |ref - f64| + 1e-5 |score|; returns the ratio |gpu - f64| / (|ref - f64| + 1e-5 |score|)"""
    eg, er = abs(float(got) - exact), abs(float(want_ref) - exact)
    print("forward %s: gpu %r ref %r f64 %r" % (name, float(got), float(want_ref), exact))
    assert eg <= 2 * er + 1e-5 * abs(exact), (name, got, want_ref, exact)
    return eg / (er + 1e-5 * abs(exact) + 1e-30)


def test_per_read_against_reference(cases):
    L = sa.lib()
    worst = 0.0
    for c in cases:
        want_s, want_p = c["ref_v"]
        got_s, got_p = call_squig(L, c["sig"], c["start"], c["end"], c["params"], c["pens"], True, gpu=True)
        assert got_s.tobytes() == want_s.tobytes(), (c["name"], got_s, want_s)
        assert np.array_equal(got_p, want_p), c["name"]
        np_s, np_p = c["np_v"]
        assert np.float32(np_s).tobytes() == got_s.tobytes() and np.array_equal(np_p, got_p[c["start"]:c["end"]]), c["name"]
        got_f, _ = call_squig(L, c["sig"], c["start"], c["end"], c["params"], c["pens"], False, gpu=True)
        worst = max(worst, _forward_ok(got_f, c["ref_f"], c["f64"], c["name"]))
    print("forward: worst |gpu - f64| / (|ref - f64| + 1e-5 |score|) = %.3f" % worst)


def test_per_read_scratch_cases(scratch_cases):
    """the scratch home through the per-read surface: Viterbi score and padded path byte for byte against the reference
    and the restatement, forward by _forward_ok"""
    L = sa.lib()
    worst = 0.0
    before = sa.launch_form_counts()["squig"]
    for c in scratch_cases:
        want_s, want_p = c["ref_v"]
        got_s, got_p = call_squig(L, c["sig"], c["start"], c["end"], c["params"], c["pens"], True, gpu=True)
        assert got_s.tobytes() == want_s.tobytes(), (c["name"], got_s, want_s)
        assert np.array_equal(got_p, want_p), c["name"]
        np_s, np_p = c["np_v"]
        assert np.float32(np_s).tobytes() == got_s.tobytes() and np.array_equal(np_p, got_p[c["start"]:c["end"]]), c["name"]
        got_f, _ = call_squig(L, c["sig"], c["start"], c["end"], c["params"], c["pens"], False, gpu=True)
        worst = max(worst, _forward_ok(got_f, c["ref_f"], c["f64"], c["name"]))
    after = sa.launch_form_counts()["squig"]
    assert after[(True, True)] - before[(True, True)] == len(scratch_cases) == after[(False, True)] - before[(False, True)]
    assert after[(True, False)] == before[(True, False)] and after[(False, False)] == before[(False, False)]
    print("forward, scratch home: worst |gpu - f64| / (|ref - f64| + 1e-5 |score|) = %.3f" % worst)


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


def test_engine_scratch_neighbours(eng, ref, cases, scratch_cases):
    """LDS and scratch reads interleaved in ONE call, the same scratch read three times with scratch reads of other sizes
    between the copies: the copies' rows sit at three offsets of one scratch allocation, beside different neighbours, and
    must give the same bytes.  Run with penalty set 1 (back states and skips) and with set 2 (no local penalty: paths
    stay in START and END, so the first and last floats of every row stay live to the last sample; two of the scratch
    reads are the all-ties squiggles of 3 and 257 samples).  Then a budget (1 MiB) that cuts the call into several
    launches -- a launch is a run of consecutive reads, the largest read nearly fills one by itself (scratch only) and
    every LDS read has a small scratch read beside it (both homes) -- and one (640 KiB) under which exactly the largest
    read's traceback does not fit.  launch_form_counts tells the launches of each home."""
    T = lds_threshold()
    lds = [next(c for c in cases if len(c["params"]) == n) for n in (64, 257, 1000, 3)]
    by = {c["name"]: c for c in scratch_cases}
    npos = sorted({len(c["params"]) for c in scratch_cases})
    win = next(c for c in scratch_cases if c["start"] > 0)
    X, first, big, mid = (by[n] for n in ("scr_p%d_s400_set1" % npos[2], "scr_p%d_s64_set1" % npos[0],
                                          "scr_p%d_s400_set1" % npos[6], "scr_p%d_s65_set1" % npos[4]))
    ties257, ties3 = by["scr_p%d_s257_set2" % npos[5]], by["scr_p%d_s3_set2" % npos[2]]
    call = [lds[0], win, lds[1], X, first, X, ties257, lds[2], big, X, mid, ties3, lds[3]]
    copies = [i for i, c in enumerate(call) if c is X]
    ibig = call.index(big)
    assert len(copies) == 3 and all(len(c["params"]) <= T for c in lds)
    assert all(len(call[i]["params"]) > T and call[i] is not X for i in (copies[0] + 1, copies[1] + 1, copies[2] - 1))
    size = [len(c["params"]) * (c["end"] - c["start"]) for c in call]
    assert size[ibig] == max(size) and size[ibig] > 2 * sorted(size)[-2]       # the traceback, samples x positions / 2 bytes, decides what fits
    rts = []
    for c in call:
        rt = sa.RawTable(c["sig"])
        rt._rt.start, rt._rt.end = c["start"], c["end"]
        rts.append(rt)
    sqs = [c["params"] for c in call]

    def delta(a, b):
        return {k: b[k] - a[k] for k in a}
    try:
        for pens in (PENS[1], PENS[2]):
            kw = dict(rate=pens[0], back_prob=pens[1], local_pen=pens[2], skip_pen=pens[3], min_score=pens[4])
            want = []
            for c in call:
                own = c["pens"] is pens
                sig, start, end, params = c["sig"], c["start"], c["end"], c["params"]
                want.append(dict(v=c["ref_v"] if own else call_squig(ref, sig, start, end, params, pens, True),
                                 f=c["ref_f"] if own else call_squig(ref, sig, start, end, params, pens, False)[0],
                                 f64=c["f64"] if own else float(np_squiggle_match(sig[start:end], params, *pens, viterbi=False, dtype=np.float64)[0])))
            fwd0 = None
            for kb, refused in ((0, False), (1024, False), (640, True)):
                eng.debug_option("squiggle_budget_kb", kb)
                c0 = sa.launch_form_counts()["squig"]
                res = eng.match_squiggle(rts, sqs, viterbi=True, path=True, **kw)
                err = sa.last_error()
                c1 = sa.launch_form_counts()["squig"]
                fwd = eng.match_squiggle(rts, sqs, viterbi=False, **kw)
                c2 = sa.launch_form_counts()["squig"]
                dv, df = delta(c0, c1), delta(c1, c2)
                assert dv[(False, False)] == dv[(False, True)] == 0 == df[(True, False)] == df[(True, True)]
                n_scr, n_lds = dv[(True, True)], dv[(True, False)]
                if kb == 0:
                    assert n_scr == 1 and n_lds == 1, dv            # one launch (the homes alternate in call order): both homes
                else:
                    assert n_scr > n_lds >= 1, dv                   # more launches with scratch reads than with LDS reads: one without LDS reads
                assert df[(False, True)] >= 1 and df[(False, False)] >= 1
                assert len(res) == len(call) == len(fwd)
                for i, (c, w, (sc, pth), (fs, fp)) in enumerate(zip(call, want, res, fwd)):
                    assert fp is None
                    if refused and i == ibig:
                        assert np.isnan(sc) and pth is None and "more than one launch may take" in err, err
                    else:
                        assert np.float32(sc).tobytes() == w["v"][0].tobytes(), (kb, i, c["name"], sc, w["v"][0])
                        assert pth is not None and np.array_equal(pth, w["v"][1]), (kb, i, c["name"])
                    _forward_ok(fs, w["f"], w["f64"], c["name"])
                a, b, c3 = (res[i] for i in copies)
                assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() == np.float32(c3[0]).tobytes()
                assert a[1].tobytes() == b[1].tobytes() == c3[1].tobytes()
                fb = [np.float32(fs).tobytes() for fs, _ in fwd]
                assert fb[copies[0]] == fb[copies[1]] == fb[copies[2]]
                if fwd0 is None:
                    fwd0 = fb
                assert fb == fwd0, kb                       # a read's forward score does not depend on its neighbours or its launch
    finally:
        eng.debug_option("squiggle_budget_kb", 0)


def test_engine_all_cases_in_one_call(eng, ref, cases):
    """every case in ONE call per parameter set: LDS and scratch homes mixed, several launches (a 1 MB budget), windows"""
    rts = []
    for c in cases:
        rt = sa.RawTable(c["sig"])
        rt._rt.start, rt._rt.end = c["start"], c["end"]
        rts.append(rt)
    sqs = [c["params"] for c in cases]
    eng.debug_option("squiggle_budget_kb", 1024)
    try:
        for pens in PENS:
            kw = dict(rate=pens[0], back_prob=pens[1], local_pen=pens[2], skip_pen=pens[3], min_score=pens[4])
            res = eng.match_squiggle(rts, sqs, viterbi=True, path=True, **kw)
            fwd = eng.match_squiggle(rts, sqs, viterbi=False, **kw)
            assert len(res) == len(cases) == len(fwd)
            for c, (sc, pth), (fs, fp) in zip(cases, res, fwd):
                own = c["pens"] is pens
                want_s, want_p = c["ref_v"] if own else call_squig(ref, c["sig"], c["start"], c["end"], c["params"], pens, True)
                assert np.float32(sc).tobytes() == want_s.tobytes(), (c["name"], pens, sc, want_s)
                assert pth is not None and np.array_equal(pth, want_p), (c["name"], pens)
                assert fp is None
                if own:
                    np_s, np_p = c["np_v"]
                    assert np.float32(np_s).tobytes() == np.float32(sc).tobytes(), c["name"]
                    assert np.array_equal(np_p, pth[c["start"]:c["end"]]), c["name"]
                    _forward_ok(fs, c["ref_f"], c["f64"], c["name"])
            t = eng.squiggle_timing()
            assert t["match_ms"] > 0 and t["walk_ms"] > 0
        # a read whose traceback cannot fit a launch: NAN for it and a text, the others as before
        eng.debug_option("squiggle_budget_kb", 256)
        res = eng.match_squiggle(rts, sqs, viterbi=True, path=True)
        big = [i for i, c in enumerate(cases) if (c["end"] - c["start"]) * ((len(c["params"]) + 63) // 64) * 32 > 256 * 1024]
        assert big and "more than one launch may take" in sa.last_error()
        for i, (c, (sc, pth)) in enumerate(zip(cases, res)):
            if i in big:
                assert np.isnan(sc) and pth is None
            elif c["pens"] is PENS[0]:
                assert np.float32(sc).tobytes() == c["ref_v"][0].tobytes() and np.array_equal(pth, c["ref_v"][1]), c["name"]
    finally:
        eng.debug_option("squiggle_budget_kb", 0)


def test_engine_failed_launch(eng, cases):
    """the second of several launches refused (debug option fail_run): the call fails with that text and hands nothing back,
    and the engine then gives what it gave before"""
    rts = []
    for c in cases:
        rt = sa.RawTable(c["sig"])
        rt._rt.start, rt._rt.end = c["start"], c["end"]
        rts.append(rt)
    sqs = [c["params"] for c in cases]
    lds_form = (True, False)                               # Viterbi, LDS: at most one launch of it per launch of the call
    eng.debug_option("squiggle_budget_kb", 256)
    try:
        before = sa.launch_form_counts()["squig"][lds_form]
        first = eng.match_squiggle(rts, sqs, viterbi=True, path=True)
        launches = sa.launch_form_counts()["squig"][lds_form] - before
        print("launches under a budget of 256 KB: at least %d" % launches)
        assert launches >= 3
        eng.debug_option("fail_run", 2)
        got = None
        with pytest.raises(RuntimeError, match="injected failure"):
            got = eng.match_squiggle(rts, sqs, viterbi=True, path=True)
        assert got is None
        eng.debug_option("fail_run", 0)
        again = eng.match_squiggle(rts, sqs, viterbi=True, path=True)
        assert len(again) == len(first)
        for c, (s0, p0), (s1, p1) in zip(cases, first, again):
            assert np.float32(s0).tobytes() == np.float32(s1).tobytes(), c["name"]
            assert (p0 is None and p1 is None) or np.array_equal(p0, p1), c["name"]
    finally:
        eng.debug_option("fail_run", 0)
        eng.debug_option("squiggle_budget_kb", 0)


def test_path_follows_the_simulated_squiggle(ref):
    params, sig, truth = synth.simulated_squiggle(400, 12)
    pens = PENS[0]
    want_s, want_p = call_squig(ref, sig, 0, len(sig), params, pens, True)
    agree_ref = float(np.mean(want_p == truth))
    L = sa.lib()
    got_s, got_p = call_squig(L, sig, 0, len(sig), params, pens, True, gpu=True)
    agree_gpu = float(np.mean(got_p == truth))
    print("agreement with the true positions: reference %.4f, gpu %.4f over %d samples" % (agree_ref, agree_gpu, len(sig)))
    assert agree_gpu == agree_ref and got_s.tobytes() == want_s.tobytes()
    assert agree_ref > 0.5
    perm = params[np.random.RandomState(3).permutation(len(params))]
    for vit in (True, False):
        true_s = call_squig(L, sig, 0, len(sig), params, pens, vit, gpu=True)[0]
        perm_s = call_squig(L, sig, 0, len(sig), perm, pens, vit, gpu=True)[0]
        assert true_s > perm_s, (vit, true_s, perm_s)


def test_map_signal_to_squiggle_on_raw_data(ref):
    params, sig, _ = synth.simulated_squiggle(300, 21)
    body = 90.0 + 12.0 * sig
    rng = np.random.RandomState(4)
    data = np.concatenate([90.0 + rng.normal(0, 1.0, 400), body, 90.0 + rng.normal(0, 1.0, 150)])
    data = np.round(data).astype(np.int16)                  # raw DAC-like values
    score, path = sa.map_signal_to_squiggle(data, params)
    rt = sa.RawTable(data).trim().scale()
    assert rt.start > 0 and rt.end < len(data) and rt.end > rt.start
    want_s, want_p = call_squig(ref, rt._data, rt.start, rt.end, params, PENS[0], True)
    assert np.float32(score).tobytes() == want_s.tobytes()
    assert len(path) == len(data) and np.array_equal(path, want_p)
    assert np.all(path[:rt.start] == -1) and np.all(path[rt.end:] == -1) and np.any(path >= 0)
    m = sa.ScrappyMatrix.from_numpy(params, sloika=False)
    score2, path2 = sa.map_signal_to_squiggle(data, m)
    assert np.float32(score2).tobytes() == want_s.tobytes() and np.array_equal(path2, want_p)
    fs, fp = sa.squiggle_match(rt, m, viterbi=False, path=False)
    assert fp is None and fs >= score - 1e-3 * abs(score)


def test_a_sequence_needs_the_predictor():
    with pytest.raises(NotImplementedError):
        sa.map_signal_to_squiggle(np.zeros(2000, dtype=np.float32), "ACGTACGTACGTACGT")
    e = sa.Engine(0)
    try:
        with pytest.raises(NotImplementedError):
            e.match_squiggle([np.zeros(100, dtype=np.float32)], ["ACGTACGT"])
    finally:
        e.close()


def test_per_read_threads(cases):
    L = sa.lib()
    some = [c for c in cases if 60 <= len(c["params"]) <= 300][:8]
    assert len(some) == 8

    def one(c):
        return call_squig(L, c["sig"], c["start"], c["end"], c["params"], c["pens"], True, gpu=True)
    alone = [one(c) for c in some]
    with ThreadPoolExecutor(8) as ex:
        together = list(ex.map(one, some))
    for (a_s, a_p), (t_s, t_p) in zip(alone, together):
        assert a_s.tobytes() == t_s.tobytes() and np.array_equal(a_p, t_p)


def test_every_squig_form_was_launched(forms_at_start):
    """the last test of the module: each of the four k_squig instantiations (Viterbi / forward x LDS / scratch) has been
    launched by the tests above"""
    now = sa.launch_form_counts()["squig"]
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("k_squig launches by (viterbi, scratch): %r" % sorted(ran.items()))
    assert len(ran) == 4 and all(v > 0 for v in ran.values()), ran
