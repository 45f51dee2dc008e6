"""Banded squiggle matching on the GPU (sh_squig_band.h, k_squig_band / k_squig_band_walk): the per-read
squiggle_match_viterbi_banded / _forward_banded, Engine.match_squiggle(band=), Engine.mappy(band=) and `scrappie mappy --band`
against the banded restatement of tests/test_squiggle_band_cpu.py -- Viterbi score and padded path bit for bit, "no path"
(restatement score < -1e29) <=> NAN -- and, where the band contains the reference's path, against the reference's compiled
unbanded code.  Forward: |gpu - f64| <= 2 |np32 - f64| + 1e-5 |score| with the float32 restatement standing in for the
reference, which has no banded form.  The sizes are those at which the band's index arithmetic can go wrong, not workloads."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_squiggle_band_cpu import band_contains, hugging_band, np_squiggle_match_banded, path_envelope
from test_squiggle_cpu import PENS, _case_inputs, _wandering_inputs, call_squig, lds_threshold, ref_squiggle_lib

pytestmark = pytest.mark.gpu

I32P = C.POINTER(C.c_int32)


def band_max_width():
    return int(sa.lib().scrappie_hip_squiggle_band_lds_max_width())


@pytest.fixture(scope="module")
def ref():
    R = ref_squiggle_lib()
    assert R is not None, "oracle/_ref/libref_decode.so is required (build() makes it and it travels with the tree)"
    return R


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """k_squig_band launches per form before this module's first test (test_every_band_form_was_launched)"""
    return sa.squiggle_band_form_counts()


def call_band(sig, start, end, params, pens, low, width, viterbi):
    """one squiggle_match_*_banded call of this build on a padded signal: (score, path_padded or None)"""
    L = sa.lib()
    sig = np.ascontiguousarray(sig, dtype=np.float32)
    import oracle
    m = oracle.NpMat(params)
    rt = sa._RawTable(None, len(sig), start, end, sig.ctypes.data_as(C.POINTER(C.c_float)))
    ptr = C.cast(m.ptr, C.POINTER(sa._Mat))
    low = np.ascontiguousarray(low, dtype=np.int32)
    if viterbi:
        path = np.full(len(sig), -7, dtype=np.int32)
        s = L.squiggle_match_viterbi_banded(rt, pens[0], ptr, *pens[1:], low.ctypes.data_as(I32P), width, path.ctypes.data_as(I32P))
        return np.float32(s), path
    return np.float32(L.squiggle_match_forward_banded(rt, pens[0], ptr, *pens[1:], low.ctypes.data_as(I32P), width)), None


# ---------------------------------------------------------------------------
# inputs and bands
# ---------------------------------------------------------------------------
def band_inputs():
    """(name, padded signal, start, end, params, pens): npos 3, 64, 65, 257, 1000, then 1819 and 4100 (beyond the unbanded LDS
    home), M + 10; samples 1, 2, 3, 64, 65, 500; the three penalty sets; a window inside a read"""
    T, M = lds_threshold(), band_max_width()
    grid = [(3, 64, 2), (3, 2, 0), (64, 65, 1), (64, 1, 0), (65, 500, 0), (257, 500, 1), (257, 2, 2), (1000, 65, 2), (1000, 500, 1),
            (1000, 3, 0), (T + 1, 64, 1), (4100, 65, 0), (4100, 3, 1), (M + 10, 65, 1), (M + 10, 2, 2)]
    out = []
    for j, (npos, ns, k) in enumerate(grid):
        params, sig = _wandering_inputs(npos, ns, 7000 + j) if k == 1 else _case_inputs(npos, ns, PENS[k], 7000 + j)
        out.append(("p%d_s%d_set%d" % (npos, ns, k), sig, 0, ns, params, PENS[k]))
    params, sig = _wandering_inputs(80, 700, 7077)
    out.append(("window_p80", sig, 100, 650, params, PENS[1]))
    return out


def diagonal_distance(path, npos):
    """the path's largest distance from the diagonal t * npos // nsample, in positions"""
    path = np.asarray(path, dtype=np.int64)
    t = np.arange(len(path), dtype=np.int64)
    m = path >= 0
    return int(np.max(np.abs(path[m] - t[m] * npos // len(path)))) if m.any() else 0


def band_shapes(win_path, npos, ns):
    """{shape: (low, width, must it contain the path)} for a window of ns samples whose reference path is win_path"""
    lo, hi = path_envelope(win_path, npos)
    hug_low, hug_w = hugging_band(win_path, npos, 0)
    shapes = {"full": (np.zeros(ns, dtype=np.int32), npos, True)}
    h = diagonal_distance(win_path, npos) + 8
    dl, dw = sa.squiggle_diagonal_band(ns, npos, h)
    shapes["diagonal"] = (dl, dw, True)
    shapes["low_edge"] = (hug_low, hug_w, True)                                   # the path runs in cell 0 wherever it is its envelope's minimum
    shapes["high_edge"] = (np.maximum(hi - (hug_w - 1), 0).astype(np.int32), hug_w, True)
    shapes["margin"] = hugging_band(win_path, npos, 37) + (True,)                 # the envelope and 37 positions either side: two ballot groups
    w = max(1, min(npos, 5 + npos // 7))
    t = np.arange(ns)
    shapes["stall_slide"] = (np.minimum(np.maximum(t - ns // 3, 0) * 3, npos - 1).astype(np.int32), w, False)      # 3 per sample: further than a skip
    shapes["jump"] = (np.where(t < (ns + 1) // 2, 0, min(npos - 1, 2 * w + 3)).astype(np.int32), w, False)        # by more than its width
    shapes["last"] = (np.full(ns, npos - 1, dtype=np.int32), 1, False)
    return shapes


def _expected(c, low, width):
    """what the restatement gives inside the band: Viterbi in float32, forward in float32 and float64"""
    x = c["sig"][c["start"]:c["end"]]
    return dict(np_v=np_squiggle_match_banded(low, width, x, c["params"], *c["pens"], viterbi=True),
                np_f=float(np_squiggle_match_banded(low, width, x, c["params"], *c["pens"], viterbi=False)[0]),
                f64=float(np_squiggle_match_banded(low, width, x, c["params"], *c["pens"], viterbi=False, dtype=np.float64)[0]))


@pytest.fixture(scope="module")
def cases(ref):
    """every input with the reference's unbanded result and, per band shape, the restatement's banded results; computed once"""
    out = []
    for name, sig, start, end, params, pens in band_inputs():
        c = dict(name=name, sig=sig, start=start, end=end, params=params, pens=pens)
        c["ref_v"] = call_squig(ref, sig, start, end, params, pens, True)
        c["bands"] = {}
        for shape, (low, width, contains) in band_shapes(c["ref_v"][1][start:end], len(params), end - start).items():
            if contains:
                assert band_contains(c["ref_v"][1][start:end], low, width), (name, shape)
            c["bands"][shape] = dict(low=low, width=width, contains=contains, **_expected(c, low, width))
        out.append(c)
    return out


def _check_viterbi(c, b, got_s, got_p, what):
    """got (score, padded path or None) against the restatement inside band b of case c, and against the reference where
    the band contains its path"""
    np_s, np_p = b["np_v"]
    start, end = c["start"], c["end"]
    if np_s < -1e29:
        assert np.isnan(got_s), (what, got_s, np_s)
        return False
    assert np.float32(np_s).tobytes() == np.float32(got_s).tobytes(), (what, got_s, np_s)
    assert got_p is not None and np.array_equal(got_p[start:end], np_p), what
    assert np.all(got_p[:start] == -1) and np.all(got_p[end:] == -1), what
    if b["contains"]:
        assert c["ref_v"][0].tobytes() == np.float32(got_s).tobytes() and np.array_equal(got_p, c["ref_v"][1]), what
    return True


def _forward_ratio(got, b, what):
    """|gpu - f64| <= 2 |np32 - f64| + 1e-5 |score|; returns |gpu - f64| / (|np32 - f64| + 1e-5 |score|)"""
    if b["np_f"] < -1e29:
        assert np.isnan(got), (what, got)
        return 0.0
    eg, er = abs(float(got) - b["f64"]), abs(b["np_f"] - b["f64"])
    print("forward %s: gpu %r np32 %r f64 %r" % (what, float(got), b["np_f"], b["f64"]))
    assert eg <= 2 * er + 1e-5 * abs(b["f64"]), (what, got, b["np_f"], b["f64"])
    return eg / (er + 1e-5 * abs(b["f64"]) + 1e-30)


# ---------------------------------------------------------------------------
# the per-read surface
# ---------------------------------------------------------------------------
def test_per_read_band_shapes(cases):
    """every input x every band shape: Viterbi bit for bit, forward within its bound; the jumping and sliding bands give a
    finite score or "no path" exactly where the restatement does; narrow bands on squiggles beyond the unbanded LDS home
    run in the banded LDS home"""
    T, M = lds_threshold(), band_max_width()
    worst, nopath, finite_loose = 0.0, 0, 0
    narrow_beyond = set()
    for c in cases:
        for shape, b in c["bands"].items():
            what = "%s/%s" % (c["name"], shape)
            before = sa.squiggle_band_form_counts()
            got_s, got_p = call_band(c["sig"], c["start"], c["end"], c["params"], c["pens"], b["low"], b["width"], True)
            ok = _check_viterbi(c, b, got_s, got_p, what)
            if not ok:
                nopath += 1
                assert "admits no path" in sa.last_error(), sa.last_error()
            elif not b["contains"]:
                finite_loose += 1
            got_f, _ = call_band(c["sig"], c["start"], c["end"], c["params"], c["pens"], b["low"], b["width"], False)
            worst = max(worst, _forward_ratio(got_f, b, what))
            after = sa.squiggle_band_form_counts()
            scratch = min(b["width"], len(c["params"])) > M
            assert after[(True, scratch)] - before[(True, scratch)] == 1 == after[(False, scratch)] - before[(False, scratch)], what
            assert after[(True, not scratch)] == before[(True, not scratch)] and after[(False, not scratch)] == before[(False, not scratch)], what
            if len(c["params"]) > T and shape not in ("full", "diagonal"):
                assert b["width"] <= M // 4 and not scratch, what     # beyond the unbanded LDS home, narrow, and in the banded one
                narrow_beyond.add(len(c["params"]))
    print("banded forward: worst |gpu - f64| / (|np32 - f64| + 1e-5 |score|) = %.3f; %d bands without a path, %d loose bands with one"
          % (worst, nopath, finite_loose))
    assert finite_loose > 0 and {T + 1, 4100} <= narrow_beyond


def test_per_read_widths():
    """widths 1, 2, 3, 63, 64, 65, 255, 256, 257 (the ballot groups and the chunks of 256 threads) on 1000 positions, and
    M, M + 1 (the last width of the LDS home, the first in scratch) on M + 10 positions with 65 and 2 samples: a diagonal
    low for that width, a band that stalls and slides, and one that hugs the high edge of the squiggle"""
    M = band_max_width()
    worst = 0.0
    todo = [(1000, 65, 1, w) for w in (1, 2, 3, 63, 64, 65, 255, 256, 257)] + [(M + 10, ns, k, w) for ns, k in ((65, 1), (2, 2), (64, 0)) for w in (M, M + 1)]
    inputs = {}
    for npos, ns, k, w in todo:
        if (npos, ns, k) not in inputs:
            inputs[npos, ns, k] = _wandering_inputs(npos, ns, 7100 + ns) if k == 1 else _case_inputs(npos, ns, PENS[k], 7100 + ns)
        params, sig = inputs[npos, ns, k]
        c = dict(name="p%d_s%d_w%d" % (npos, ns, w), sig=sig, start=0, end=ns, params=params, pens=PENS[k])
        t = np.arange(ns, dtype=np.int64)
        lows = {"diag": np.clip(t * npos // ns - w // 2, 0, npos - w), "from0": np.minimum(t // 2, npos - 1),
                "slide": np.minimum(np.maximum(t - ns // 2, 0) * 3, npos - 1), "top": np.minimum(npos - w + t // 8, npos - 1)}
        for shape, low in lows.items():
            low = low.astype(np.int32)
            b = dict(low=low, width=w, contains=False, **_expected(c, low, w))
            what = "%s/%s" % (c["name"], shape)
            before = sa.squiggle_band_form_counts()
            got_s, got_p = call_band(sig, 0, ns, params, PENS[k], low, w, True)
            _check_viterbi(c, b, got_s, got_p, what)
            got_f, _ = call_band(sig, 0, ns, params, PENS[k], low, w, False)
            worst = max(worst, _forward_ratio(got_f, b, what))
            after = sa.squiggle_band_form_counts()
            assert after[(True, w > M)] == before[(True, w > M)] + 1 and after[(True, w <= M)] == before[(True, w <= M)], what
    print("banded forward over the widths: worst ratio %.3f" % worst)


def test_python_layer(cases, ref):
    """sa.squiggle_match(band=): an int is the diagonal half-width, a pair is used as given, a band without a path raises"""
    c = next(c for c in cases if c["name"].startswith("window"))
    rt = sa.RawTable(c["sig"])
    rt._rt.start, rt._rt.end = c["start"], c["end"]
    kw = dict(rate=c["pens"][0], back_prob=c["pens"][1], local_pen=c["pens"][2], skip_pen=c["pens"][3], min_score=c["pens"][4])
    b = c["bands"]["diagonal"]
    h = diagonal_distance(c["ref_v"][1][c["start"]:c["end"]], len(c["params"])) + 8
    assert sa.squiggle_diagonal_band(c["end"] - c["start"], len(c["params"]), h)[1] == b["width"]
    for band in (h, (b["low"], b["width"])):
        s, p = sa.squiggle_match(rt, c["params"], band=band, **kw)
        assert np.float32(s).tobytes() == c["ref_v"][0].tobytes() and np.array_equal(p, c["ref_v"][1])
    fs, fp = sa.squiggle_match(rt, c["params"], viterbi=False, path=False, band=h, **kw)
    assert fp is None and abs(fs - b["f64"]) <= 2 * abs(b["np_f"] - b["f64"]) + 1e-5 * abs(b["f64"])
    # a band that jumps from positions 0..2 to 60..62: whatever the restatement says of it, a score or no path
    params, sig = _case_inputs(80, 40, PENS[0], 5)
    low = np.where(np.arange(40) < 20, 0, 60).astype(np.int32)
    want = np_squiggle_match_banded(low, 3, sig, params, *PENS[0])
    if want[0] < -1e29:
        with pytest.raises(RuntimeError, match="admits no path"):
            sa.squiggle_match(sa.RawTable(sig), params, band=(low, 3))
    else:
        s, p = sa.squiggle_match(sa.RawTable(sig), params, band=(low, 3))
        assert np.float32(s).tobytes() == np.float32(want[0]).tobytes() and np.array_equal(p, want[1])


def test_simulated_read_in_a_diagonal_band(ref):
    """a simulated read of a few thousand samples: inside the diagonal band of the helper the path is the unbanded path"""
    params, sig, truth = synth.simulated_squiggle(500, 12)
    assert 2000 < len(sig) < 8000
    pens = PENS[0]
    want_s, want_p = call_squig(ref, sig, 0, len(sig), params, pens, True)
    h = diagonal_distance(want_p, len(params)) + 8
    low, width = sa.squiggle_diagonal_band(len(sig), len(params), h)
    assert width < len(params) and band_contains(want_p, low, width)
    got_s, got_p = call_band(sig, 0, len(sig), params, pens, low, width, True)
    assert got_s.tobytes() == want_s.tobytes() and np.array_equal(got_p, want_p)
    un_s, un_p = call_squig(sa.lib(), sig, 0, len(sig), params, pens, True, gpu=True)
    assert un_s.tobytes() == got_s.tobytes() and np.array_equal(un_p, got_p)
    assert float(np.mean(got_p == truth)) > 0.5


# ---------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


def _raw_table(c):
    rt = sa.RawTable(c["sig"])
    rt._rt.start, rt._rt.end = c["start"], c["end"]
    return rt


def test_engine_mixed_call(eng, cases):
    """ONE call mixing banded reads of the LDS home, of the scratch home and unbanded reads, one banded read three times
    between others (identical bytes); then budgets that cut the call into several launches; Viterbi and forward"""
    M = band_max_width()
    by = {c["name"]: c for c in cases}
    big, p1000, p257, win, p4100 = (by[n] for n in ("p%d_s65_set1" % (M + 10), "p1000_s500_set1", "p257_s500_set1", "window_p80", "p4100_s65_set0"))
    X = (p1000, "diagonal")
    call = [(p257, "low_edge"), X, (p257, "margin"), (big, "full"), (p257, None), X, (win, "high_edge"), (p4100, "full"), (win, None), X,
            (p4100, "low_edge"), (p1000, "stall_slide"), (big, "stall_slide"), (p1000, None)]
    copies = [i for i, x in enumerate(call) if x is X]
    assert len(copies) == 3
    n_scr = sum(1 for c, s in call if s is not None and min(c["bands"][s]["width"], len(c["params"])) > M)
    assert n_scr == 2 and sum(1 for c, s in call if s is None) == 3
    rts = [_raw_table(c) for c, s in call]
    sqs = [c["params"] for c, s in call]
    bands = [None if s is None else (c["bands"][s]["low"], c["bands"][s]["width"]) for c, s in call]
    pens = PENS[1]
    kw = dict(rate=pens[0], back_prob=pens[1], local_pen=pens[2], skip_pen=pens[3], min_score=pens[4])
    want = []
    for (c, s), rt in zip(call, rts):
        x = c["sig"][c["start"]:c["end"]]
        low, width = (np.zeros(len(x), dtype=np.int32), len(c["params"])) if s is None else (c["bands"][s]["low"], c["bands"][s]["width"])
        own = c["pens"] is pens and s is not None
        want.append(dict(np_v=c["bands"][s]["np_v"] if own else np_squiggle_match_banded(low, width, x, c["params"], *pens),
                         np_f=c["bands"][s]["np_f"] if own else float(np_squiggle_match_banded(low, width, x, c["params"], *pens, viterbi=False)[0]),
                         f64=c["bands"][s]["f64"] if own else float(np_squiggle_match_banded(low, width, x, c["params"], *pens, viterbi=False, dtype=np.float64)[0]),
                         contains=False))
    fwd0 = None
    try:
        for kb in (0, 1024, 600):
            eng.debug_option("squiggle_budget_kb", kb)
            b0, u0 = sa.squiggle_band_form_counts(), sa.launch_form_counts()["squig"]
            res = eng.match_squiggle(rts, sqs, viterbi=True, path=True, band=bands, **kw)
            b1, u1 = sa.squiggle_band_form_counts(), sa.launch_form_counts()["squig"]
            t = eng.squiggle_timing()
            assert t["match_ms"] > 0 and t["walk_ms"] > 0 and t["tables_ms"] > 0
            fwd = eng.match_squiggle(rts, sqs, viterbi=False, band=bands, **kw)
            b2 = sa.squiggle_band_form_counts()
            lds_l, scr_l = b1[(True, False)] - b0[(True, False)], b1[(True, True)] - b0[(True, True)]
            assert b1[(False, False)] == b0[(False, False)] and b1[(False, True)] == b0[(False, True)]
            assert b2[(False, False)] > b1[(False, False)] and b2[(False, True)] > b1[(False, True)] and b2[(True, False)] == b1[(True, False)]
            assert u1[(True, False)] > u0[(True, False)] and u1[(True, True)] == u0[(True, True)]      # the unbanded reads: k_squig, LDS home
            if kb == 0:
                assert lds_l == 1 and scr_l == 1, (lds_l, scr_l)          # one banded launch: both homes
            else:
                assert lds_l + scr_l >= 3, (kb, lds_l, scr_l)             # cut into several
            assert len(res) == len(call) == len(fwd)
            for i, ((c, s), w, (sc, pth), (fs, fp)) in enumerate(zip(call, want, res, fwd)):
                what = "kb %d read %d %s/%s" % (kb, i, c["name"], s)
                assert fp is None
                assert _check_viterbi(c, w, np.float32(sc), pth, what), what
                _forward_ratio(fs, w, what)
            a, b, c3 = (res[i] for i in copies)
            assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() == np.float32(c3[0]).tobytes()
            assert a[1].tobytes() == b[1].tobytes() == c3[1].tobytes()
            fb = [np.float32(fs).tobytes() for fs, _ in fwd]
            if fwd0 is None:
                fwd0 = fb
            assert fb == fwd0, kb                       # a read's forward score does not depend on its neighbours or its launch
    finally:
        eng.debug_option("squiggle_budget_kb", 0)


def test_engine_band_fits_where_the_full_traceback_does_not(eng, cases, ref):
    """under one budget a read is refused unbanded for its size and mapped with a band; a band list with None, an int
    for all reads, an invalid band and one without a path leave the other reads untouched"""
    c = next(c for c in cases if c["name"] == "p1000_s500_set1")
    small = next(c for c in cases if c["name"] == "p64_s65_set1")
    b = c["bands"]["margin"]
    full_bytes = 500 * 8 * ((1000 + 63) // 64) * 4
    band_bytes = sa.plan_squiggle_band([1000], [b["width"]], [500])["bytes"]
    kb = 128
    assert band_bytes < kb * 1024 < full_bytes, (band_bytes, full_bytes)
    kw = dict(rate=PENS[1][0], back_prob=PENS[1][1], local_pen=PENS[1][2], skip_pen=PENS[1][3], min_score=PENS[1][4])
    rts, sqs = [_raw_table(small), _raw_table(c), _raw_table(small)], [small["params"], c["params"], small["params"]]
    try:
        eng.debug_option("squiggle_budget_kb", kb)
        res = eng.match_squiggle(rts, sqs, viterbi=True, path=True, **kw)
        assert np.isnan(res[1][0]) and res[1][1] is None and "more than one launch may take" in sa.last_error()
        for i in (0, 2):
            assert np.float32(res[i][0]).tobytes() == small["ref_v"][0].tobytes() and np.array_equal(res[i][1], small["ref_v"][1])
        res = eng.match_squiggle(rts, sqs, viterbi=True, path=True, band=[None, (b["low"], b["width"]), None], **kw)
        assert np.float32(res[1][0]).tobytes() == c["ref_v"][0].tobytes() and np.array_equal(res[1][1], c["ref_v"][1])
        for i in (0, 2):
            assert np.float32(res[i][0]).tobytes() == small["ref_v"][0].tobytes() and np.array_equal(res[i][1], small["ref_v"][1])
    finally:
        eng.debug_option("squiggle_budget_kb", 0)
    # one int for all reads: each read's own diagonal band
    h = 1000                                                       # at least both squiggles' lengths: the full band
    res = eng.match_squiggle(rts, sqs, viterbi=True, path=True, band=h, **kw)
    for cc, (sc, pth) in zip((small, c, small), res):
        assert np.float32(sc).tobytes() == cc["ref_v"][0].tobytes() and np.array_equal(pth, cc["ref_v"][1])
    # an invalid band, and a band without a path (one sample, and its band does not hold the last position): NAN for them, the neighbour as before
    one = next(cc for cc in cases if cc["name"] == "p64_s1_set0")
    jb = one["bands"]["jump"]
    gap_want = np_squiggle_match_banded(jb["low"], jb["width"], one["sig"], one["params"], *PENS[1])
    assert gap_want[0] < -1e29
    bad = b["low"].copy(); bad[10] = bad[9] + 2; bad[11] = bad[9]
    res = eng.match_squiggle([_raw_table(one), rts[1], rts[2]], [one["params"], sqs[1], sqs[2]], viterbi=True, path=True,
                             band=[(jb["low"], jb["width"]), (bad, b["width"]), None], **kw)
    assert np.isnan(res[0][0]) and res[0][1] is None and "admits no path" in sa.last_error()      # the first refusal in input order
    assert np.isnan(res[1][0]) and res[1][1] is None
    assert np.float32(res[2][0]).tobytes() == small["ref_v"][0].tobytes() and np.array_equal(res[2][1], small["ref_v"][1])
    res = eng.match_squiggle([rts[1], rts[2]], [sqs[1], sqs[2]], viterbi=False, band=[(bad, b["width"]), None], **kw)
    assert np.isnan(res[0][0]) and "decreases" in sa.last_error() and np.isfinite(res[1][0])


def test_per_read_threads(cases):
    """the per-read banded functions from four threads at once"""
    some = [(c, s) for c in cases if 60 <= len(c["params"]) <= 1000 and c["end"] - c["start"] >= 64 for s in ("diagonal", "stall_slide")][:8]
    assert len(some) == 8

    def one(cs):
        c, s = cs
        return call_band(c["sig"], c["start"], c["end"], c["params"], c["pens"], c["bands"][s]["low"], c["bands"][s]["width"], True)
    alone = [one(x) for x in some]
    with ThreadPoolExecutor(4) as ex:
        together = list(ex.map(one, some))
    for (a_s, a_p), (t_s, t_p) in zip(alone, together):
        assert a_s.tobytes() == t_s.tobytes() and np.array_equal(a_p, t_p)


# ---------------------------------------------------------------------------
# scrappie mappy --band
# ---------------------------------------------------------------------------
READ = "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand"


@pytest.fixture(scope="module")
def mappy_setup(fast5_dir, tmp_path_factory):
    """a synthetic squiggle model in a file, a bundled read and its sequence, and `run`: scrappie mappy with options -> stdout"""
    from test_sqnet_cpu import CLI, ROOT, weights
    name = "squiggle_r94"
    mf = str(tmp_path_factory.mktemp("band_models") / (name + ".scrm"))
    model.save_model(weights(name), mf)
    fa = os.path.join(ROOT, "tests", "golden", "reads", READ + ".fa")
    f5 = os.path.join(fast5_dir, READ + ".fast5")
    seq = "".join(l.strip() for l in open(fa).read().splitlines()[1:])

    def run(*opts, ok=True):
        r = subprocess.run([CLI, "mappy", "--model-file", mf] + list(opts) + [fa, f5], capture_output=True, text=True, timeout=120)
        assert (r.returncode == 0) == ok, r.stderr
        return r.stdout if ok else r.stderr
    return dict(name=name, mf=mf, fa=fa, f5=f5, seq=seq, run=run)


def test_cli_mappy_wide_band_is_no_band(mappy_setup):
    """`scrappie mappy --band N` with N >= the squiggle's length: byte-equal to the run without the option"""
    m = mappy_setup
    plain = m["run"]()
    assert plain.startswith("# ") and len(plain.splitlines()) > 1000
    assert m["run"]("--band", str(len(m["seq"]))) == plain
    assert "--band" in m["run"]("--band", "-3", ok=False)          # refused while the options are read


def test_cli_mappy_narrow_band_is_engine_mappy(mappy_setup):
    """`scrappie mappy --band=5`: the score and path of Engine.mappy(band=5) on the trimmed and scaled read, which differ from the
    unbanded ones or equal them as the engine says"""
    m = mappy_setup
    L = sa.lib()
    rt = L.scrappie_hip_read_raw(os.fsencode(m["f5"]), True)
    raw = np.ctypeslib.as_array(rt.raw, shape=(rt.n,)).copy()
    sa._libc.free(C.cast(rt.raw, C.c_void_p))
    trimmed = sa.RawTable(raw).trim().scale()
    e = sa.Engine(0)
    try:
        e.load_model(m["name"], m["mf"])
        (score, path), = e.mappy([trimmed], [m["seq"]], model=m["name"], band=5)
    finally:
        e.close()
    assert np.isfinite(score) and path is not None
    lines = m["run"]("--band=5").splitlines()
    assert lines[0] == "# %s to %s  (score = %f)" % (m["f5"], m["fa"], score)
    assert lines[1] == "idx\tsignal\tpos\tbase\tcurrent\tsd\tdwell" and len(lines) == 2 + len(raw)
    pos = np.array([int(l.split("\t")[2]) for l in lines[2:]])
    assert np.array_equal(pos, path)
    low, width = sa.squiggle_diagonal_band(trimmed.end - trimmed.start, len(m["seq"]), 5)
    inside = pos[trimmed.start:trimmed.end]
    assert width == 11 and np.all((inside == -1) | ((inside >= low) & (inside < low + width)))


def test_every_band_form_was_launched(forms_at_start):
    """the last test of the module: each of the four k_squig_band instantiations (Viterbi / forward x LDS / scratch) has been
    launched by the tests above"""
    now = sa.squiggle_band_form_counts()
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("k_squig_band launches by (viterbi, scratch): %r" % sorted(ran.items()))
    assert len(ran) == 4 and all(v > 0 for v in ran.values()), ran
