"""Squiggle matching (squiggle_match_viterbi / _forward, map_signal_to_squiggle) without a GPU.

The second pin of the squiggle-matching kernel lives here: `np_squiggle_match`, a numpy restatement of the two recursions
of decode.c:1016-1401, vectorised over positions, with its per-position tables from the host's libm through ctypes (so
they carry the bits the reference's own expf / tanhf / logf / log1pf give).  In float32 its Viterbi score and path must
equal the reference's compiled code (oracle/_ref/libref_decode.so) byte for byte on every case of `squig_cases`;
tests/test_gpu_squiggle.py holds the GPU against both.  Also here: the argument errors of the per-read functions (NAN
and a text, before any GPU work), the case generator's own coverage and `synth.simulated_squiggle`."""
import ctypes as C
import ctypes.util
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import scrappie_amd as sa
from scrappie_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = np.float32(1e30)
M_LN2 = 0.693147180559945309417232121458176568

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _nm in ("expf", "tanhf", "logf", "log1pf"):
    getattr(_libm, _nm).restype = C.c_float
    getattr(_libm, _nm).argtypes = [C.c_float]


# ---------------------------------------------------------------------------
# numpy restatement of decode.c:1016-1401
# ---------------------------------------------------------------------------
def _lse(x, y):
    """util.h:162-164 in the array's own precision"""
    return np.fmax(x, y) + np.log1p(np.exp(-np.abs(x - y)))


def _tables(par, rate, prob_back, dtype):
    """decode.c:1055-1099: (loc, logsc, scale, move_pen[npos + 2], stay_pen[npos + 2], move_back_pen, half_pen); float32
    from libm with the reference's expressions and summation order, float64 from numpy on the same float32 inputs"""
    npos = len(par)
    if np.dtype(dtype) == np.float64:
        p = par.astype(np.float64)
        r, pb = np.float64(np.float32(rate)), np.float64(np.float32(prob_back))
        mp = (1.0 - pb) * (0.5 * (1.0 + np.tanh((p[:, 2] + np.log(r)) / 2.0)))
        mv, sy = np.log(mp), np.log1p(-mp - pb)
        move = np.concatenate(([mv.mean()], mv, [mv.mean()]))
        stay = np.concatenate(([sy.mean()], sy, [sy.mean()]))
        return p[:, 0], p[:, 1], np.exp(p[:, 1]), move, stay, np.log(pb), np.log(np.float64(0.5))
    f = np.float32
    pb = f(prob_back)
    scale = np.array([_libm.expf(float(v)) for v in par[:, 1]], dtype=f)
    lograte = f(_libm.logf(float(f(rate))))
    move, stay = np.zeros(npos + 2, dtype=f), np.zeros(npos + 2, dtype=f)
    mean_move, mean_stay = f(0), f(0)
    for pos in range(npos):
        x = f(par[pos, 2] + lograte)
        mp = f(f(f(1) - pb) * f(f(0.5) * f(f(1) + f(_libm.tanhf(float(f(x / f(2))))))))
        move[pos + 1] = _libm.logf(float(mp))
        stay[pos + 1] = _libm.log1pf(float(f(f(-mp) - pb)))
        mean_move = f(mean_move + move[pos + 1])
        mean_stay = f(mean_stay + stay[pos + 1])
    move[0] = move[npos + 1] = f(mean_move / f(npos))
    stay[0] = stay[npos + 1] = f(mean_stay / f(npos))
    return par[:, 0], par[:, 1], scale, move, stay, f(_libm.logf(float(pb))), f(_libm.logf(0.5))


def np_squiggle_match(signal, params, rate, prob_back, local_pen, skip_pen, minscore, viterbi=True, dtype=np.float32):
    """(score, path or None): signal the samples that are mapped (the window, not the padded read); params (npos, 3)
    float32 (mean, log sd, dwell logit).  The path has one entry per sample, recoded as decode.c:1210-1234."""
    f = np.dtype(dtype).type
    x = np.asarray(signal, dtype=np.float32).astype(dtype)
    par = np.ascontiguousarray(params, dtype=np.float32)
    NP, ns = len(par), len(x)
    NF = NP + 2
    NST = NF + NP
    with np.errstate(all="ignore"):
        loc, logsc, scale, move, stay, back_pen, half = _tables(par, rate, prob_back, dtype)
        loc, logsc, scale = loc.astype(dtype), logsc.astype(dtype), scale.astype(dtype)
        lp, kp, ms = f(np.float32(local_pen)), f(np.float32(skip_pen)), f(np.float32(minscore))
        dest = np.arange(1, NP).astype(dtype)              # destpos of START -> sequence
        delta = (NP - np.arange(1, NP)).astype(dtype)      # deltapos of sequence -> END, by origst
        c = np.full(NST, -f(BIG), dtype=dtype)
        c[0] = 0
        tb = np.zeros((ns, NST), dtype=np.int32) if viterbi else None
        for t in range(ns):
            p, c = c, np.empty_like(c)
            c[:NF] = p[:NF] + stay
            c[NF:] = p[NF:] + half
            step = p[:NF - 1] + move[:NF - 1]
            skip = (p[:NF - 2] + move[:NF - 2]) - kp
            fs = (p[0] + move[0]) - lp * dest
            cand = (p[1:NP] + move[1:NP]) - lp * delta
            mb = p[2:NP + 1] + back_pen
            fb = p[NF:NF + NP - 1] + half
            if viterbi:
                src = np.arange(NST, dtype=np.int32)
                m = step > c[1:NF]
                c[1:NF] = np.where(m, step, c[1:NF]); src[1:NF] = np.where(m, np.arange(NF - 1), src[1:NF])
                m = skip > c[2:NF]
                c[2:NF] = np.where(m, skip, c[2:NF]); src[2:NF] = np.where(m, np.arange(NF - 2), src[2:NF])
                m = fs > c[2:NP + 1]
                c[2:NP + 1] = np.where(m, fs, c[2:NP + 1]); src[2:NP + 1] = np.where(m, 0, src[2:NP + 1])
                if NP > 1:
                    k = int(np.argmax(cand))               # the first maximum, as the ascending loop of strict > keeps it
                    if cand[k] > c[NF - 1]:
                        c[NF - 1] = cand[k]; src[NF - 1] = k + 1
                m = mb > c[NF:NF + NP - 1]
                c[NF:NF + NP - 1] = np.where(m, mb, c[NF:NF + NP - 1])
                src[NF:NF + NP - 1] = np.where(m, np.arange(2, NP + 1), src[NF:NF + NP - 1])
                m = fb > c[2:NP + 1]
                c[2:NP + 1] = np.where(m, fb, c[2:NP + 1]); src[2:NP + 1] = np.where(m, np.arange(NF, NF + NP - 1), src[2:NP + 1])
                tb[t] = src
            else:
                c[1:NF] = _lse(c[1:NF], step)
                c[2:NF] = _lse(c[2:NF], skip)
                c[2:NP + 1] = _lse(c[2:NP + 1], fs)
                if NP > 1:                                  # (the order of END's sum is free)
                    top = np.max(cand)
                    c[NF - 1] = _lse(c[NF - 1], top + np.log(np.sum(np.exp(cand - top))))
                c[NF:NF + NP - 1] = _lse(c[NF:NF + NP - 1], mb)
                c[2:NP + 1] = _lse(c[2:NP + 1], fb)
            e = -np.abs(x[t] - loc) / scale - logsc
            e = np.fmax(-ms, (e.astype(np.float64) - M_LN2).astype(dtype))
            c[1:NP + 1] += e
            c[NF:] += e
            c[0] -= lp
            c[NF - 1] -= lp
        if not viterbi:
            return _lse(c[NF - 2], c[NF - 1]), None
        score = np.fmax(c[NF - 2], c[NF - 1])
    path = np.zeros(ns, dtype=np.int64)
    path[-1] = NF - 2 if c[NF - 2] > c[NF - 1] else NF - 1
    for t in range(ns - 1, 0, -1):
        path[t - 1] = tb[t, path[t]]
    lo, hi = 0, ns                                         # decode.c:1210-1234, literally
    while lo < ns and path[lo] == 0:
        path[lo] = -1; lo += 1
    while hi > 0 and path[hi - 1] == NF - 1:
        path[hi - 1] = -1; hi -= 1
    for t in range(lo, hi):
        assert path[t] > 0
        path[t] -= NF if path[t] >= NF else 1
    return score, path.astype(np.int32)


# ---------------------------------------------------------------------------
# the compiled reference, and one call of either library
# ---------------------------------------------------------------------------
def ref_squiggle_lib():
    R = oracle.ref_decode()
    if R is None:
        return None
    PM = C.POINTER(oracle.Mat)
    R.squiggle_match_viterbi.restype = C.c_float
    R.squiggle_match_viterbi.argtypes = [oracle.RawTable, C.c_float, PM, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int32)]
    R.squiggle_match_forward.restype = C.c_float
    R.squiggle_match_forward.argtypes = [oracle.RawTable, C.c_float, PM, C.c_float, C.c_float, C.c_float, C.c_float]
    return R


def call_squig(L, sig, start, end, params, pens, viterbi, gpu=False):
    """one squiggle_match_* call of library L (the reference, or this build with gpu=True) on a padded signal:
    (score, path_padded or None)"""
    sig = np.ascontiguousarray(sig, dtype=np.float32)
    m = oracle.NpMat(params)
    RT = sa._RawTable if gpu else oracle.RawTable
    rt = RT(None, len(sig), start, end, sig.ctypes.data_as(C.POINTER(C.c_float)))
    ptr = C.cast(m.ptr, C.POINTER(sa._Mat)) if gpu else m.ptr
    if viterbi:
        path = np.full(len(sig), -7, dtype=np.int32)
        s = L.squiggle_match_viterbi(rt, pens[0], ptr, *pens[1:], path.ctypes.data_as(C.POINTER(C.c_int32)))
        return np.float32(s), path
    return np.float32(L.squiggle_match_forward(rt, pens[0], ptr, *pens[1:])), None


# ---------------------------------------------------------------------------
# the cases both pins are checked on
# ---------------------------------------------------------------------------
NPOS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000)
NSAMPLE = (1, 2, 3, 64, 65, 500, 1501)
# (rate, prob_back, local_pen, skip_pen, minscore): scrappy's defaults; back states and skips live; exact ties
PENS = [(1.0, 0.0, 2.0, 5000.0, 5.0), (0.7, 0.1, 2.0, 5.0, 5.0), (1.3, 0.05, 0.0, 0.0, 0.25)]


def grid_pairs(T):
    """(npos, nsample): every npos with two sample counts, every nsample with at least two npos; T - 1, T, T + 1 (the
    kernel's LDS-to-scratch threshold) with 40 and 41 samples, one of each ping-pong parity"""
    pairs = []
    for i, npos in enumerate(NPOS):
        pairs += [(npos, NSAMPLE[i % 7]), (npos, NSAMPLE[(i + 3) % 7])]
    for npos in (T - 1, T, T + 1):
        pairs += [(npos, 40), (npos, 41)]
    return pairs


def _case_inputs(npos, ns, pens, seed):
    if pens is PENS[2]:
        # one parameter triple for all positions and every emission on the -minscore floor (|x| + ln 2 > 0.25 always):
        # all paths of equal move counts tie exactly and the first-maximum order decides
        params = np.tile(np.array([[0.0, 0.0, -1.5]], dtype=np.float32), (npos, 1))
        sig = np.random.RandomState(seed).normal(0.0, 1.0, size=ns).astype(np.float32)
        return params, sig
    params, sig, _ = synth.simulated_squiggle(npos, seed, mean_dwell=max(2.0, min(8.0, ns / npos)))
    if len(sig) < ns:
        sig = np.tile(sig, ns // len(sig) + 1)
    return params, np.ascontiguousarray(sig[:ns])


def squig_cases(T):
    """(name, padded signal, start, end, params, pens)"""
    out = []
    for j, (npos, ns) in enumerate(grid_pairs(T)):
        pens = PENS[j % 3]
        params, sig = _case_inputs(npos, ns, pens, 1000 + j)
        out.append(("p%d_s%d_set%d" % (npos, ns, j % 3), sig, 0, ns, params, pens))
    params, sig = _case_inputs(80, 700, PENS[1], 77)          # a window inside a longer read: the padding
    out.append(("window_p80", sig, 100, 650, params, PENS[1]))
    return out


def lds_threshold():
    L = sa.lib()
    return int(L.scrappie_hip_squiggle_lds_max_pos())


# ---------------------------------------------------------------------------
# the scratch home: squiggles of more than T positions, whose rows live in device scratch and whose tables are read from
# global memory (sh_squig.h).  squig_cases reaches it at T + 1 only, with the two uninformative penalty sets.
# ---------------------------------------------------------------------------
SCRATCH_NSAMPLE = (1, 2, 3, 64, 65, 257, 400)


def scratch_npos(T):
    """T + 1; the next multiple of 64 and one past it; the next multiple of 256 (a chunk of the kernel's 256 threads more)
    -1 / 0 / +1; about 2.25 T.  For T = 1818: 1819, 1856, 1857, 2047, 2048, 2049, 4100."""
    r64 = (T + 2 + 63) // 64 * 64
    r256 = (r64 + 2 + 255) // 256 * 256
    return (T + 1, r64, r64 + 1, r256 - 1, r256, r256 + 1, (9 * T // 4 + 99) // 100 * 100)


def scratch_grid(T):
    """(npos, nsample, index into PENS): two sample counts of opposite parity per npos, every count and every set used"""
    n = scratch_npos(T)
    return [(n[0], 1, 0), (n[0], 64, 1), (n[1], 2, 2), (n[1], 65, 0), (n[2], 3, 2), (n[2], 400, 1), (n[3], 64, 2),
            (n[3], 257, 1), (n[4], 65, 1), (n[4], 400, 0), (n[5], 257, 2), (n[5], 2, 0), (n[6], 400, 1), (n[6], 3, 2)]


def _wandering_inputs(npos, ns, seed):
    """simulated_squiggle's parameters and a signal that walks them from position 0 with what PENS[1] keeps alive: skipped
    positions and excursions one position back (k + 1, k, k + 1: through back state k), two samples at each stop so that
    the excursion pays for its two penalties"""
    params, _, _ = synth.simulated_squiggle(npos, seed, mean_dwell=2.0)
    rng = np.random.RandomState(seed + 1)
    walk = []
    pos = 0
    while len(walk) < ns:
        walk += [pos, pos]
        r = rng.rand()
        if r < 0.15 and pos >= 1:
            walk += [pos - 1, pos - 1, pos, pos]
        pos = min(pos + (2 if 0.15 <= r < 0.30 else 1), npos - 1)
    walk = np.array(walk[:ns])
    sig = params[walk, 0] + rng.laplace(0.0, 1.0, size=ns) * np.exp(params[walk, 1])
    return params, sig.astype(np.float32)


def squig_scratch_cases(T):
    """(name, padded signal, start, end, params, pens): scratch_grid, and a window inside a longer read"""
    out = []
    for j, (npos, ns, k) in enumerate(scratch_grid(T)):
        params, sig = _wandering_inputs(npos, ns, 3000 + j) if k == 1 else _case_inputs(npos, ns, PENS[k], 3000 + j)
        out.append(("scr_p%d_s%d_set%d" % (npos, ns, k), sig, 0, ns, params, PENS[k]))
    npos = scratch_npos(T)[5]
    params, sig = _wandering_inputs(npos, 257, 3077)
    pad = np.random.RandomState(5).normal(0.0, 1.0, size=500).astype(np.float32)
    pad[70:327] = sig
    out.append(("scr_window_p%d" % npos, pad, 70, 327, params, PENS[1]))
    return out


def path_moves(path):
    """(backward steps, skips) of a recoded Viterbi path: position differences < 0 and == 2 between mapped samples"""
    d = np.diff(path[path >= 0])
    return int(np.sum(d < 0)), int(np.sum(d == 2))


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_scratch_cases_cover_the_scratch_home():
    T = lds_threshold()
    grid = scratch_grid(T)
    npos = scratch_npos(T)
    assert len(set(grid)) == len(grid) and len(set(npos)) == 7 and all(n > T for n in npos)
    if T == 1818:
        assert npos == (1819, 1856, 1857, 2047, 2048, 2049, 4100)
    assert npos[0] == T + 1 and npos[1] % 64 == 0 and npos[2] == npos[1] + 1
    assert npos[4] % 256 == 0 and npos[3] == npos[4] - 1 and npos[5] == npos[4] + 1       # the chunk boundary of 256 threads
    assert (npos[3] + 255) // 256 + 1 == (npos[5] + 255) // 256
    assert 2.2 * T < npos[6] < 2.3 * T and (npos[6] + 255) // 256 >= 2 * ((npos[0] + 255) // 256)
    for n in npos:
        ss = [s for p, s, k in grid if p == n]
        assert len(ss) == 2 and (ss[0] + ss[1]) % 2 == 1, n                      # both ping-pong parities
    assert {s for p, s, k in grid} == set(SCRATCH_NSAMPLE)
    for k in range(3):
        assert sum(1 for g in grid if g[2] == k) >= 2, k
    assert sum(1 for g in grid if g[2] == 1) >= 3 and (npos[6], 400, 1) in grid
    for p, s, k in grid:
        assert s * (2 * p + 2) * 4 < 50e6                                         # the reference's traceback
    cases = squig_scratch_cases(T)
    assert len(cases) == len(grid) + 1 and len({c[0] for c in cases}) == len(cases)
    for name, sig, start, end, params, pens in cases:
        assert len(params) > T and sig.dtype == np.float32 and params.dtype == np.float32, name      # every one is the scratch form
    wins = [c for c in cases if c[2] > 0 and c[3] < len(c[1])]
    assert len(wins) == 1 and wins[0][5] is PENS[1]
    assert {c[5] for c in cases} == set(PENS)


def test_scratch_plan_keeps_neighbours_apart():
    """squig_plan_add: k_squig touches 2 (2 npos + 1) floats from a read's scratch offset (both rows: START, the positions
    and the back states).  The sizes of scratch_npos, T + 1 ... T + 5, LDS reads between them, several orders."""
    from test_map_cpu import check_scratch_plan
    T = lds_threshold()
    npos = [T + 1, T + 2, 5, T + 3, T, T + 4, T + 5] + list(scratch_npos(T)) + [T - 1, T + 1, 1 << 20]
    rng = np.random.default_rng(29)
    for order in (np.arange(len(npos)), np.arange(len(npos))[::-1], rng.permutation(len(npos)), rng.permutation(len(npos))):
        P = [npos[i] for i in order]
        check_scratch_plan("squig", P, [SCRATCH_NSAMPLE[i % 7] for i in range(len(P))], lambda n: n <= T, lambda n: 2 * (2 * n + 1))
    for n in (T + 1, T + 2, T + 3, T + 4):
        check_scratch_plan("squig", [n], [64], lambda m: m <= T, lambda m: 2 * (2 * m + 1))


@pytest.mark.parametrize("viterbi", [True, False])
def test_restatement_equals_reference_scratch_cases(viterbi):
    """as test_restatement_equals_reference on squig_scratch_cases; and some PENS[1] path there goes through a back state,
    some through a skip"""
    R = ref_squiggle_lib()
    if R is None:
        pytest.skip("oracle/_ref/libref_decode.so not built")
    nback = nskip = 0
    for name, sig, start, end, params, pens in squig_scratch_cases(lds_threshold()):
        want_s, want_p = call_squig(R, sig, start, end, params, pens, viterbi)
        got_s, got_p = np_squiggle_match(sig[start:end], params, *pens, viterbi=viterbi)
        if viterbi:
            assert np.float32(got_s).tobytes() == want_s.tobytes(), (name, got_s, want_s)
            assert np.all(want_p[:start] == -1) and np.all(want_p[end:] == -1), name
            assert np.array_equal(got_p, want_p[start:end]), name
            if pens is PENS[1]:
                b, k = path_moves(want_p)
                nback += b; nskip += k
        else:
            assert abs(float(got_s) - float(want_s)) <= 1e-5 * abs(float(want_s)) + 1e-3, (name, got_s, want_s)
    if viterbi:
        assert nback > 0 and nskip > 0, (nback, nskip)


def test_case_grid_covers_the_sizes():
    T = lds_threshold()
    assert 256 < T < 65536
    pairs = grid_pairs(T)
    assert len(set(pairs)) == len(pairs)
    for npos in NPOS + (T - 1, T, T + 1):
        assert len({s for p, s in pairs if p == npos}) == 2, npos
    for ns in NSAMPLE:
        assert len({p for p, s in pairs if s == ns}) >= 2, ns
    for npos, ns in pairs:
        assert ns * (2 * npos + 2) * 4 < 50e6                 # the reference's traceback
    cases = squig_cases(T)
    assert {c[5] for c in cases} == set(PENS)
    assert any(c[2] > 0 and c[3] < len(c[1]) for c in cases)


@pytest.mark.parametrize("viterbi", [True, False])
def test_restatement_equals_reference(viterbi):
    """the numpy restatement against decode.c as compiled: Viterbi byte for byte (score and padded path), forward within
    float32 rounding"""
    R = ref_squiggle_lib()
    if R is None:
        pytest.skip("oracle/_ref/libref_decode.so not built")
    nback = 0
    for name, sig, start, end, params, pens in squig_cases(lds_threshold()):
        want_s, want_p = call_squig(R, sig, start, end, params, pens, viterbi)
        got_s, got_p = np_squiggle_match(sig[start:end], params, *pens, viterbi=viterbi)
        if viterbi:
            assert np.float32(got_s).tobytes() == want_s.tobytes(), (name, got_s, want_s)
            assert np.all(want_p[:start] == -1) and np.all(want_p[end:] == -1), name
            assert np.array_equal(got_p, want_p[start:end]), name
            inside = got_p[got_p >= 0]
            nback += int(np.sum(np.diff(inside) < 0))
        else:
            assert abs(float(got_s) - float(want_s)) <= 1e-5 * abs(float(want_s)) + 1e-3, (name, got_s, want_s)
    if viterbi:
        assert nback > 0          # some case walks through a back state


def test_argument_errors_without_gpu():
    """where the reference asserts or is undefined: NAN and a text, and nothing is launched (this runs without a GPU)"""
    L = sa.lib()
    params, sig, _ = synth.simulated_squiggle(10, 1)
    good = (1.0, 0.0, 2.0, 5000.0, 5.0)

    def both(sig, start, end, params, pens, word):
        for vit in (True, False):
            s, _ = call_squig(L, sig, start, end, params, pens, vit, gpu=True)
            assert np.isnan(s), (word, vit)
            assert word in sa.last_error(), (word, sa.last_error())

    both(sig, 0, len(sig), params, (0.0,) + good[1:], "rate")
    both(sig, 0, len(sig), params, (-1.0,) + good[1:], "rate")
    both(sig, 0, len(sig), params, (1.0, -0.1) + good[2:], "prob_back")
    both(sig, 0, len(sig), params, (1.0, 1.5) + good[2:], "prob_back")
    both(sig, 5, 5, params, good, "empty")
    both(sig, 7, 3, params, good, "empty")
    both(sig, 0, len(sig) + 1, params, good, "past")
    PM = C.POINTER(sa._Mat)
    rt = sa._RawTable(None, len(sig), 0, len(sig), sig.ctypes.data_as(C.POINTER(C.c_float)))
    path = np.zeros(len(sig), dtype=np.int32)
    pp = path.ctypes.data_as(C.POINTER(C.c_int32))
    m = oracle.NpMat(params)
    mp = C.cast(m.ptr, PM)
    empty = sa._Mat(3, 1, 0, 4, m.mat.data)                    # npos == 0
    assert np.isnan(L.squiggle_match_viterbi(rt, *good[:1], C.pointer(empty), *good[1:], pp)) and "no positions" in sa.last_error()
    assert np.isnan(L.squiggle_match_forward(rt, *good[:1], C.pointer(empty), *good[1:]))
    assert np.isnan(L.squiggle_match_viterbi(rt, good[0], None, *good[1:], pp)) and "squiggle" in sa.last_error()
    assert np.isnan(L.squiggle_match_viterbi(rt, good[0], mp, *good[1:], None)) and "path" in sa.last_error()
    null = sa._RawTable(None, len(sig), 0, len(sig), None)
    assert np.isnan(L.squiggle_match_forward(null, good[0], mp, *good[1:])) and "signal" in sa.last_error()
    # the Python layer: a base sequence needs the predictor, which is not built
    with pytest.raises(NotImplementedError):
        sa.map_signal_to_squiggle(np.zeros(1000, dtype=np.float32), "ACGTACGT")
    with pytest.raises(ValueError):
        sa.squiggle_match(sa.RawTable(sig), params, viterbi=False, path=True)
    with pytest.raises(ValueError):
        sa.squiggle_match(sa.RawTable(sig), params[:, :2])


def test_simulated_squiggle_is_deterministic():
    a, b = synth.simulated_squiggle(200, 5), synth.simulated_squiggle(200, 5)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    params, sig, truth = a
    assert params.shape == (200, 3) and params.dtype == np.float32 and sig.dtype == np.float32
    assert len(sig) == len(truth) and truth[0] == 0 and truth[-1] == 199 and np.all(np.diff(truth) >= 0)
    assert 5.0 < len(sig) / 200 < 12.0                         # mean_dwell = 8
    assert abs(float(np.mean(params[:, 1])) - np.log(0.15)) < 0.05
    assert not np.array_equal(synth.simulated_squiggle(200, 6)[1][:50], sig[:50])
    p4, s4, _ = synth.simulated_squiggle(200, 5, mean_dwell=4.0)
    assert 2.5 < len(s4) / 200 < 6.0


def test_pyscrap_squiggle_cdef_links(tmp_path):
    """include/pyscrap_squiggle.h: both prototypes agree with scrappie_hip.h and link against the built library alone"""
    text = open(os.path.join(ROOT, "include", "pyscrap_squiggle.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    names = re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*\(", text)
    assert sorted(names) == ["squiggle_match_forward", "squiggle_match_viterbi"]
    src = tmp_path / "link.c"
    src.write_text('#include "scrappie_hip.h"\n' + text + "\nvoid *table[] = {" + ", ".join("(void *)" + n for n in names) +
                   "};\nint main(void) { return table[0] == 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "link"),
                        "-L", os.path.join(ROOT, "scrappie_amd"), "-lscrappie_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "scrappie_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
