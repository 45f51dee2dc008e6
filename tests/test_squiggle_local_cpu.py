"""A raw signal mapped INTO a longer reference squiggle (k_squig_local, sh_squig_local.h), the part that needs no GPU: the numpy
restatement np_squiggle_local -- the authority for the definition, which the reference project does not have -- with the same cut
into windows and the same order of the end reduction as the kernel, the five arguments that hold the definition, placements of
simulated signals, the window planner (scrappie_hip_squiggle_local_plan, csrc/sh_host.c), the argument errors of the per-read
functions and tests/squiggle_local_asan.c, a program of its own over sh_host.c under the address and undefined-behaviour sanitizers.

The definition is squiggle_match_viterbi / _forward (decode.c:1016-1401; np_squiggle_match in test_squiggle_cpu.py) with the squiggle
side made local: the move out of START enters every position and one END accumulator per position lets every position leave, both
without a distance term; START has no step or skip of its own.
  1. Ownership: a path enters the squiggle from START once, at p0, advances at most 2 positions per sample and reaches at most one
     cell to the left (back state p0 - 1); window w of stride s owns the paths with p0 in [w s, (w + 1) s) and holds the cells they
     can be in; a path's score is the same chain of additions wherever it is computed: the Viterbi score has the same bits for
     every stride.
  2. Every path of the reference's definition is a path here and pays no less there (local_pen >= 0): local >= reference.
  3. With local_pen = 0 and skip_pen >= 0 the reference's distance terms vanish, its END step and skip are dominated, and
     fl(max(a_i) + b) = max fl(a_i + b) makes one END per position the shared END: a path that ends in END scores the compiled
     reference's bits.
  4. A float64 brute force over all paths, maximum and log-sum.
  5. Float64 forward: the windows sum to the one window."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import oracle
import scrappie_amd as sa
from scrappie_amd import synth
from test_map_local_cpu import _reduce
from test_squiggle_cpu import M_LN2, PENS, _case_inputs, _lse, _tables, call_squig, np_squiggle_match, ref_squiggle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1e30
LDS_BYTES = 65536               # SH_SQ_LDS
SCR_MUL = 4                     # SH_SQUIG_LOCAL_SCR_MUL: entry positions per sample a window in device scratch owns at the default stride
# (rate, prob_back, local_pen, skip_pen, minscore): the three of test_squiggle_cpu.py, and back states and skips alive with local_pen = 0
PENS4 = list(PENS) + [(0.7, 0.1, 0.0, 5.0, 5.0)]
END_SETS = ((0.7, 0.1, 0.0, 5.0, 5.0), (1.3, 0.05, 0.0, 0.0, 5.0), (1.0, 0.0, 0.0, 5000.0, 5.0))      # local_pen = 0, skip_pen >= 0, minscore 5
WANDER = (0.7, 0.1, 2.0, 5.0, 5.0)      # what keeps skips and back excursions alive (PENS[1])
NEW_SYMBOLS = ("squiggle_match_local_viterbi", "squiggle_match_local_forward", "scrappie_hip_squiggle_match_local_batch",
               "scrappie_hip_free_squiggle_local_results", "scrappie_hip_squiggle_local_plan", "scrappie_hip_squiggle_local_stride",
               "scrappie_hip_squiggle_local_max_cells", "scrappie_hip_squiggle_local_form_counts")


def need_feature():
    """(every test begins here: without the symbols it fails, it does not skip)"""
    for name in NEW_SYMBOLS:
        assert hasattr(sa.lib(), name), name


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def lds_bytes(ncell):
    """a head of 16 words; two rows of a position and a back value per cell, the END row, loc / scale / logsc / stay per cell and
    ncell + 2 move entries"""
    return (16 + 10 * ncell + 2) * 4


def max_cells():
    return (LDS_BYTES - lds_bytes(0)) // 40


def scr_floats(ncell):
    return (5 * ncell + 3) // 4 * 4


def np_stride(L, ns, stride):
    """stride > 0: entry positions per window; 0 or None: one window; < 0: the default"""
    reach, M = 2 * (ns - 1) + 1, max_cells()
    if stride is None or stride == 0:
        s = L
    elif stride > 0:
        s = stride
    elif 2 * reach <= M:
        s = M - reach
    else:
        s = SCR_MUL * ns
    return min(max(s, 1), L)


def np_plan(L, ns, stride):
    """[(first cell, ncell, first owned cell in the window, own)] per window"""
    s = np_stride(L, ns, stride)
    out = []
    for p0 in range(0, L, s):
        c0 = max(p0 - 1, 0)
        end = min(p0 + s + 2 * (ns - 1), L)
        out.append((c0, end - c0, p0 - c0, min(s, L - p0)))
    return out


def _window(x, tabs, pens, c0, ncell, own0, own, viterbi, dtype, want_tb=False):
    """one window: cells c0 .. c0 + ncell - 1, of which own0 .. own0 + own - 1 take the START move.  Returns (score, end position,
    ends in E, CODE, BBIT, FRESH, TIE)"""
    f = np.dtype(dtype).type
    loc, logsc, scale, move, stay, back_pen, half = tabs
    L, ns = len(loc), len(x)
    big = f(BIG)
    lp, kp, ms = f(np.float32(pens[2])), f(np.float32(pens[3])), f(np.float32(pens[4]))
    pos = c0 + np.arange(ncell)
    mine = (np.arange(ncell) >= own0) & (np.arange(ncell) < own0 + own)
    lo, sc, lg = loc[pos].astype(dtype), scale[pos].astype(dtype), logsc[pos].astype(dtype)
    mv0, mvm, mvp, sty = move[pos].astype(dtype), move[np.maximum(pos - 1, 0)].astype(dtype), move[pos + 1].astype(dtype), stay[pos + 1].astype(dtype)
    move0, stay0, stayE = f(move[0]), f(stay[0]), f(stay[L + 1])
    back_pen, half = f(back_pen), f(half)
    c = np.full(ncell, -big, dtype=dtype)
    cb = np.full(ncell, -big, dtype=dtype)
    E = np.full(ncell, -big, dtype=dtype)
    start = f(0)
    if want_tb:
        CODE, BBIT = np.zeros((ns, ncell), dtype=np.int8), np.zeros((ns, ncell), dtype=bool)
        FRESH, TIE = np.zeros((ns, ncell), dtype=bool), np.zeros((ns + 1, 3, ncell), dtype=bool)
    else:
        CODE = BBIT = FRESH = TIE = None
    l1, l2 = np.array([-big], dtype=dtype), np.array([-big, -big], dtype=dtype)
    with np.errstate(all="ignore"):
        for t in range(ns):
            p, pb = c, cb
            p1 = np.concatenate((l1, p[:-1]))                # outside the window: no owned path
            p2 = np.concatenate((l2, p[:-2]))[:ncell]
            pr = np.concatenate((p[1:], l1))
            b1 = np.concatenate((l1, pb[:-1]))
            em = -np.abs(x[t] - lo) / sc - lg
            em = np.fmax(-ms, (em.astype(np.float64) - M_LN2).astype(dtype))
            v = p + sty
            s1, s2, fs, fb = p1 + mv0, (p2 + mvm) - kp, f(start + move0), b1 + half
            bk, mb = pb + half, pr + back_pen
            e, ex = E + stayE, p + mvp
            if viterbi:
                v0, bk0 = v, bk
                code = np.zeros(ncell, dtype=np.int8)
                for k, (ok, cand) in enumerate(((pos >= 1, s1), (pos >= 2, s2), (mine, fs), (pos >= 1, fb))):
                    m = ok & (cand > v)
                    v = np.where(m, cand, v); code = np.where(m, k + 1, code)
                bbit = (pos <= L - 2) & (mb > bk)
                bk = np.where(bbit, mb, bk)
                fresh = ex > e
                e = np.where(fresh, ex, e)
                if want_tb:
                    CODE[t], BBIT[t], FRESH[t] = code, bbit, fresh
                    neq = (v0 == v).astype(int) + ((pos >= 1) & (s1 == v)) + ((pos >= 2) & (s2 == v)) + (mine & (fs == v)) + ((pos >= 1) & (fb == v))
                    TIE[t, 0] = (neq > 1) & (v > -big / 2)
                    TIE[t, 1] = (pos <= L - 2) & (mb == bk0) & (bk > -big / 2)
                    TIE[t, 2] = (ex == (E + stayE)) & (e > -big / 2)
            else:
                v = np.where(pos >= 1, _lse(v, s1), v)
                v = np.where(pos >= 2, _lse(v, s2), v)
                v = np.where(mine, _lse(v, fs), v)
                v = np.where(pos >= 1, _lse(v, fb), v)
                bk = np.where(pos <= L - 2, _lse(bk, mb), bk)
                e = _lse(e, ex)
            c = (v + em).astype(dtype)
            cb = (bk + em).astype(dtype)
            E = (e - lp).astype(dtype)
            start = f(f(start + stay0) - lp)
        xs, kx = _reduce(c, viterbi, dtype)
        ys, ky = _reduce(E, viterbi, dtype)
        if not viterbi:
            return _lse(xs, ys), None, None, None, None, None, None
    in_e = not (xs > ys)
    k = ky if in_e else kx
    if want_tb:
        TIE[ns, 0, k] = (xs == ys) or int(((E if in_e else c) == (ys if in_e else xs)).sum()) > 1
    return np.fmax(xs, ys), c0 + k, in_e, CODE, BBIT, FRESH, TIE


def np_squiggle_local(signal, params, rate, prob_back, local_pen, skip_pen, minscore, stride=None, viterbi=True, dtype=np.float32, info=None):
    """The specification.  signal: the samples that are mapped (the window of the read); params (L, 3) float32.  The entry positions
    are cut into windows of `stride` each (None or 0: one window; -1: the default), each computed alone; the highest window, the
    lowest on a tie -- forward: _lse over the windows in their order.  Returns (score, first, last, path): path[t] the position (a
    back state as its position) or -1 in START / END, first the lowest position on it, last the end cell's position + 1; forward:
    (score, None, None, None).  info (a dict): 'tie_free' -- no two equal candidates met anywhere on the path; 'ends_in_end'."""
    x = np.asarray(signal, dtype=np.float32).astype(dtype)
    par = np.ascontiguousarray(params, dtype=np.float32)
    L, ns = len(par), len(x)
    assert L >= 1 and ns >= 1
    pens = (rate, prob_back, local_pen, skip_pen, minscore)
    with np.errstate(all="ignore"):
        tabs = _tables(par, rate, prob_back, dtype)
    plan = np_plan(L, ns, stride)
    res = [_window(x, tabs, pens, c0, nc, o0, own, viterbi, dtype) for c0, nc, o0, own in plan]
    if not viterbi:
        acc = res[0][0]
        for r in res[1:]:
            acc = _lse(acc, r[0])
        return acc, None, None, None
    scores = np.array([r[0] for r in res], dtype=dtype)
    w = int(np.argmax(scores))
    c0, nc, o0, own = plan[w]
    score, pe, in_e, CODE, BBIT, FRESH, TIE = _window(x, tabs, pens, c0, nc, o0, own, True, dtype, want_tb=True)
    assert np.asarray(score).tobytes() == np.asarray(res[w][0]).tobytes() and (pe, in_e) == (res[w][1], res[w][2])
    path = np.full(ns, -1, dtype=np.int32)
    j, st = pe - c0, (1 if in_e else 0)                      # 0: the position of cell j, 1: its E, 2: START, 3: its back state
    tie = bool(TIE[ns, 0, j]) or int((scores == scores[w]).sum()) > 1
    for t in range(ns - 1, -1, -1):
        if st in (0, 3):
            path[t] = c0 + j
        if st == 1:
            tie = tie or bool(TIE[t, 2, j])
            if FRESH[t, j]:
                st = 0
        elif st == 0:
            tie = tie or bool(TIE[t, 0, j])
            code = int(CODE[t, j])
            if code == 3:
                st = 2
            elif code == 4:
                st, j = 3, j - 1
            else:
                j -= code
            assert j >= 0
        elif st == 3:
            tie = tie or bool(TIE[t, 1, j])
            if BBIT[t, j]:
                st, j = 0, j + 1
    assert st == 2
    on = path[path >= 0]
    assert len(on) >= 1 and c0 + o0 <= on[0] < c0 + o0 + own      # it entered where the window owns
    if info is not None:
        info["tie_free"] = not tie
        info["ends_in_end"] = bool(in_e)
    return score, int(on.min()), int(pe) + 1, path


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def walk_inputs(L, a, b, seed, lead=0, trail=0, clip=None, plain=0):
    """simulated_squiggle's parameters for L positions and a signal that walks positions a .. b - 1 of them with what WANDER keeps
    alive, in the style of test_squiggle_cpu._wandering_inputs: two samples at each stop, skipped positions, excursions one position
    back; `lead` / `trail` samples far from every level in front and behind; clip: the noise draws are kept within that many noise
    scales; plain: the first and last that many stops are plain steps.  Returns (params, signal, the walk)"""
    params, _, _ = synth.simulated_squiggle(L, seed, mean_dwell=2.0)
    rng = np.random.RandomState(seed + 1)
    walk, pos = [], a
    while True:
        walk += [pos, pos]
        if pos == b - 1:
            break
        r = rng.rand()
        if pos < a + plain or pos + 2 > b - 1 - plain:
            r = 1.0
        if r < 0.15 and pos >= a + 1:
            walk += [pos - 1, pos - 1, pos, pos]
        pos = min(pos + (2 if 0.15 <= r < 0.30 else 1), b - 1)
    walk = np.array(walk)
    noise = rng.laplace(0.0, 1.0, size=len(walk))
    if clip is not None:
        noise = np.clip(noise, -clip, clip)
    sig = params[walk, 0] + noise * np.exp(params[walk, 1])
    sig = np.concatenate((np.full(lead, 50.0), sig, np.full(trail, 50.0)))
    return params, sig.astype(np.float32), walk


def local_cases():
    """(name, signal, params, index into PENS4): L 1 .. 130, 5 .. 66 samples, every penalty set"""
    shapes = ((1, 5), (2, 5), (3, 6), (4, 9), (7, 5), (9, 20), (20, 9), (30, 30), (17, 64), (64, 17), (40, 66), (65, 65), (130, 33), (100, 12),
              (70, 40), (25, 26), (8, 7), (3, 8), (63, 10), (129, 50), (5, 66), (33, 33))
    out = []
    for i, (L, ns) in enumerate(shapes):
        for k in (i % 4, (i + 1) % 4):
            if k == 2:
                params, sig = _case_inputs(L, ns, PENS[2], 500 + i)
            elif k in (1, 3) and L >= 4:
                a = (i * 7) % max(L // 2, 1)
                params, sig, _ = walk_inputs(L, a, L if i % 3 == 0 else max(a + 2, L - i % 5), 500 + i)
                sig = np.resize(sig, ns)
            else:
                params, sig = _case_inputs(L, ns, PENS[0], 500 + i)
            out.append(("L%d_s%d_set%d" % (L, ns, k), sig, params, k))
    return out


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    need_feature()
    assert set(sa.squiggle_local_form_counts()) == {(v, s) for v in (False, True) for s in (False, True)}
    M = max_cells()
    assert sa.squiggle_local_max_cells() == M == 1636
    assert lds_bytes(M) <= LDS_BYTES < lds_bytes(M + 1)
    assert (M - 1) // 2 + 1 == 818                       # a window holds at least 2 (ns - 1) + 1 cells: the LDS home ends at 818 samples
    assert set(sa.squiggle_band_form_counts()) == {(v, s) for v in (False, True) for s in (False, True)}      # the others' counters, as before


def test_case_list_covers_the_ground():
    need_feature()
    cases = local_cases()
    assert len(cases) == 44 and len({c[0] for c in cases}) == 44
    assert {c[3] for c in cases} == {0, 1, 2, 3}
    assert min(len(c[2]) for c in cases) == 1 and max(len(c[2]) for c in cases) == 130
    assert min(len(c[1]) for c in cases) == 5 and max(len(c[1]) for c in cases) == 66


def test_every_stride_gives_the_one_window_bits():
    """argument 1: strides 1, 3, 7, 64, the default and one window give the score's bits; first, last and the path wherever the
    one-window run met no tie"""
    need_feature()
    n = free = 0
    for name, sig, params, k in local_cases():
        info = {}
        s0, f0, l0, p0 = np_squiggle_local(sig, params, *PENS4[k], info=info)
        n += 1
        free += info["tie_free"]
        for stride in (1, 3, 7, 64, -1, len(params)):
            s, f, l, p = np_squiggle_local(sig, params, *PENS4[k], stride=stride)
            assert np.float32(s).tobytes() == np.float32(s0).tobytes(), (name, stride, s, s0)
            if info["tie_free"]:
                assert (f, l) == (f0, l0) and np.array_equal(p, p0), (name, stride)
    print("tie-free cases: %d of %d" % (free, n))
    assert n == 44 and free >= n // 2


def test_local_is_never_below_the_reference_definition():
    """argument 2: every path of squiggle_match_viterbi is a path here and pays no less there"""
    need_feature()
    n = 0
    for name, sig, params, k in local_cases():
        assert PENS4[k][2] >= 0
        g = np_squiggle_match(sig, params, *PENS4[k], viterbi=True)[0]
        s = np_squiggle_local(sig, params, *PENS4[k])[0]
        assert np.float32(s) >= np.float32(g), (name, s, g)
        n += 1
    assert n == 44


def test_without_local_penalty_an_end_in_end_scores_the_compiled_reference():
    """argument 3, against oracle/_ref/libref_decode.so: local_pen = 0, skip_pen >= 0, and two samples at 50.0 -- far from every
    level -- behind every signal, so that both sides end in END (asserted, no case skipped): the one-window score is the
    reference's bit for bit; the paths wherever the restatement met no tie.  The sets are END_SETS: 50.0 is far only where
    minscore makes it so -- a sample there costs minscore in a position and stay[END] (about 0.3) in END, which a path enters for
    one move (about 1.5) -- so PENS[2], whose minscore is 0.25, appears with minscore 5."""
    need_feature()
    R = ref_squiggle_lib()
    if R is None:
        pytest.skip("oracle/_ref/libref_decode.so not built")
    n = same_path = 0
    for name, sig, params, k in local_cases():
        for pens in END_SETS:
            assert pens[2] == 0.0 and pens[3] >= 0.0
            x = np.concatenate((sig, np.float32([50.0, 50.0]))).astype(np.float32)
            want_s, want_p = call_squig(R, x, 0, len(x), params, pens, True)
            info = {}
            s, first, last, path = np_squiggle_local(x, params, *pens, info=info)
            assert info["ends_in_end"] and path[-1] == -1 and np.any(path >= 0), name
            assert want_p[-1] == -1 and np.any(want_p >= 0), name
            assert np.float32(s).tobytes() == want_s.tobytes(), (name, pens, s, want_s)
            if info["tie_free"]:
                assert np.array_equal(path, want_p), (name, pens)
                same_path += 1
            n += 1
    assert n == 44 * len(END_SETS) and same_path >= 1


def _brute(x, tabs, pens, L):
    """all paths over the states START, positions, back states and one END per position, float64: (maximum, log-sum)"""
    loc, logsc, scale, move, stay, back_pen, half = tabs
    lp, kp, ms = (np.float64(np.float32(v)) for v in pens[2:])
    ns = len(x)
    em = np.fmax(-ms, -np.abs(x[:, None] - loc[None, :]) / scale[None, :] - logsc[None, :] - M_LN2)      # [t][pos]
    S, P, B, E = 0, 1, 2, 3

    def moves(kind, i):
        """(state, weight without the emission, emitting position or None)"""
        if kind == S:
            yield (S, 0), stay[0] - lp, None
            for j in range(L):
                yield (P, j), move[0], j
        elif kind == P:
            yield (P, i), stay[i + 1], i
            if i + 1 < L:
                yield (P, i + 1), move[i + 1], i + 1
            if i + 2 < L:
                yield (P, i + 2), move[i + 1] - kp, i + 2
            if i >= 1:
                yield (B, i - 1), back_pen, i - 1
            yield (E, i), move[i + 1] - lp, None
        elif kind == B:
            yield (B, i), half, i
            yield (P, i + 1), half, i + 1
        else:
            yield (E, i), stay[L + 1] - lp, None

    totals = []

    def go(t, state, acc):
        if t == ns:
            if state[0] in (P, E):
                totals.append(acc)
            return
        for nxt, w, epos in moves(*state):
            if w == -np.inf:
                continue
            go(t + 1, nxt, acc + w + (em[t, epos] if epos is not None else 0.0))

    go(0, (S, 0), 0.0)
    totals = np.array(totals)
    top = totals.max()
    return top, top + math.log(np.sum(np.exp(totals - top)))


def test_brute_force_over_all_paths():
    """argument 4: L <= 4, at most 4 samples, float64: the maximum and the log-sum over every path, to 1e-10"""
    need_feature()
    rng = np.random.RandomState(3)
    n = 0
    with np.errstate(all="ignore"):
        for L, ns in itertools.product((1, 2, 3, 4), (1, 2, 3, 4)):
            params, _, _ = synth.simulated_squiggle(L, 40 + L, mean_dwell=2.0)
            x = (params[rng.randint(0, L, ns), 0] + 0.2 * rng.standard_normal(ns)).astype(np.float32)
            for pens in PENS4 + [(1.0, 0.3, 0.5, 0.7, 5.0)]:
                tabs = _tables(params, pens[0], pens[1], np.float64)
                vmax, vsum = _brute(x.astype(np.float64), tabs, pens, L)
                for stride in (None, 1, 2):
                    got_v = np_squiggle_local(x, params, *pens, stride=stride, dtype=np.float64)[0]
                    got_f = np_squiggle_local(x, params, *pens, stride=stride, viterbi=False, dtype=np.float64)[0]
                    assert abs(float(got_v) - vmax) <= 1e-10 * max(1.0, abs(vmax)), (L, ns, pens, stride, got_v, vmax)
                    assert abs(float(got_f) - vsum) <= 1e-10 * max(1.0, abs(vsum)), (L, ns, pens, stride, got_f, vsum)
                    n += 1
    assert n == 16 * 5 * 3


def test_forward_windows_partition_the_paths():
    """argument 5, float64: the windows' forward scores sum to the one window's"""
    need_feature()
    n = 0
    for name, sig, params, k in local_cases():
        one = float(np_squiggle_local(sig, params, *PENS4[k], viterbi=False, dtype=np.float64)[0])
        for stride in (1, 3, 7, 64, -1):
            got = float(np_squiggle_local(sig, params, *PENS4[k], stride=stride, viterbi=False, dtype=np.float64)[0])
            assert abs(got - one) <= 1e-10 * max(1.0, abs(one)), (name, stride, got, one)
            n += 1
    assert n == 220


# (L, a, b, lead, trail): deep inside the reference (a well past every stride used), at position 0, ending at L - 1, with samples
# in START and END around.  a and b are nominal: see clear_ends
PLACEMENTS = ((120, 37, 61, 0, 0), (120, 0, 25, 0, 0), (120, 90, 120, 0, 0), (300, 200, 230, 3, 4), (300, 150, 170, 0, 5), (64, 20, 44, 2, 0))


def clear_ends(params, a, b):
    """Where a walk begins and ends can only be read off a signal if the level there differs from its neighbours' by more than the
    noise (simulated_squiggle: levels ~ N(0, 1), noise scale 0.15; two neighbours 0.05 apart cannot be told apart by two samples).
    So a moves right and b left -- unless they are the reference's own ends, which stay -- to the nearest position whose level is
    more than 0.5 (three noise scales) from those of the positions within 2 of it.  For the same reason the placements' noise is
    clipped at 2 noise scales: a sample then scores at least 1.2 - 2 = -0.8 in its own position (-|d| - log sd - ln 2 with log sd =
    -1.9), above the 2.3 that a sample in START or END costs, where an unclipped Laplace tail (one draw in 30 is beyond 3.4
    scales) makes START the better explanation of a first sample.  And the placements' walks begin and end with three plain steps:
    a skip costs 5 and an excursion back 2.3 + 0.7, so right at an end a detour through a neighbour of similar level -- entering
    later, leaving earlier -- can be the cheaper explanation of the same samples; in the interior it cannot.  Properties of the
    inputs alone."""
    L = len(params)
    loc = params[:, 0]

    def clear(k):
        return all(abs(float(loc[k]) - float(loc[j])) > 0.5 for j in range(max(k - 2, 0), min(k + 3, L)) if j != k)
    if a > 0:
        while not clear(a):
            a += 1
    if b < L:
        while not clear(b - 1):
            b += 1
    assert b - a >= 8 and b <= L
    return a, b


@pytest.mark.parametrize("place", PLACEMENTS, ids=lambda p: "L%d_%d_%d" % p[:3])
def test_placements_are_found(place):
    """a signal simulated from positions a .. b - 1 of a longer reference is found there: last - 1 is the walk's last position, first
    within 2 of a; the reference's definition pays local_pen per position of distance and scores far lower"""
    need_feature()
    L, a, b, lead, trail = place
    seed = 900 + L + a
    a, b = clear_ends(synth.simulated_squiggle(L, seed, mean_dwell=2.0)[0], a, b)
    params, sig, walk = walk_inputs(L, a, b, seed, lead, trail, clip=2.0, plain=3)
    assert walk[0] == a and walk[-1] == b - 1
    res = {}
    for stride in (None, 7, 64, -1):
        s, first, last, path = np_squiggle_local(sig, params, *WANDER, stride=stride)
        assert last - 1 == b - 1, (place, stride, first, last)
        assert abs(first - a) <= 2, (place, stride, first, last)
        assert np.all(path[:lead] == -1) and (trail == 0 or np.all(path[len(sig) - trail:] == -1))
        res[stride] = (np.float32(s).tobytes(), first, last)
    assert len(set(res.values())) == 1
    g = np_squiggle_match(sig, params, *WANDER, viterbi=True)[0]
    s = np_squiggle_local(sig, params, *WANDER)[0]
    if a >= 20 or L - b >= 20:
        assert float(s) - float(g) > 20.0, (place, s, g)


def test_walks_wander():
    """the placements' walks hold skips and excursions back, as WANDER keeps alive"""
    need_feature()
    nback = nskip = 0
    for L, a, b, lead, trail in PLACEMENTS:
        walk = walk_inputs(L, a, b, 900 + L + a, plain=3)[2]
        nback += int(np.sum(np.diff(walk) < 0)); nskip += int(np.sum(np.diff(walk) == 2))
    assert nback > 0 and nskip > 0


def test_smallest_shapes():
    """one sample: the best single entry; L = 1: no step, no back state; a window of one owned cell behind the back state's cell"""
    need_feature()
    rng = np.random.RandomState(17)
    for L in (1, 2, 3, 9):
        params, _, _ = synth.simulated_squiggle(L, 70 + L, mean_dwell=2.0)
        x = params[rng.randint(0, L, 1), 0].astype(np.float32)
        for pens in PENS4:
            s, first, last, path = np_squiggle_local(x, params, *pens)
            assert last == first + 1 and path.tolist() == [first]
            for stride in (1, 2):
                assert np.float32(np_squiggle_local(x, params, *pens, stride=stride)[0]).tobytes() == np.float32(s).tobytes()
    assert np_plan(5, 1, 1) == [(0, 1, 0, 1), (0, 2, 1, 1), (1, 2, 1, 1), (2, 2, 1, 1), (3, 2, 1, 1)]


def check_plan(L, ns, stride):
    pl = sa.squiggle_local_plan(L, ns, stride)
    s = int(sa.lib().scrappie_hip_squiggle_local_stride(L, ns, stride))
    assert s == np_stride(L, ns, stride), (L, ns, stride)
    want = np_plan(L, ns, stride)
    nw = len(pl["first"])
    assert nw == len(want) and nw >= 1
    at = 0
    for w in range(nw):
        first, ncell, own = int(pl["first"][w]), int(pl["ncell"][w]), int(pl["own"][w])
        assert (first, ncell, own) == (want[w][0], want[w][1], want[w][3]), (L, ns, stride, w)
        assert first == max(at - 1, 0) and own >= 1          # every entry position 0 .. L - 1 is owned exactly once; one cell to the left is kept
        assert first + ncell - 1 == min(at + s - 1 + 2 * (ns - 1), L - 1)
        at += own
        assert int(pl["home"][w]) == (1 if lds_bytes(ncell) > LDS_BYTES else 0), (L, ns, stride, w)
    assert at == L
    end = 0
    for w in range(nw):
        off = int(pl["scr_off"][w])
        if not pl["home"][w]:
            assert off == -1
            continue
        assert off % 4 == 0 and off >= end, (L, ns, stride, w)          # 16-byte aligned, disjoint
        end = off + scr_floats(int(pl["ncell"][w]))
    assert pl["scr_floats"] == end
    return pl


def test_planner():
    need_feature()
    M = max_cells()
    for L in (1, 2, 5, 63, 64, 300, 5000, 3 * M + 11):
        for ns in (1, 2, 7, 64, 409, 410, 818, 819, M + 40):
            for stride in (1, 7, 64, L + 5, 0, -1, 3000, M, M + 1):
                if stride == 1 and L > 300:
                    continue
                check_plan(L, ns, stride)
    pl = check_plan(M, 1, 0)                                  # max_cells and one more choose the two homes
    assert pl["home"].tolist() == [0] and int(pl["ncell"][0]) == M
    pl = check_plan(M + 1, 1, 0)
    assert pl["home"].tolist() == [1] and pl["scr_floats"] == scr_floats(M + 1)
    pl = check_plan(100000, 100, -1)                          # a short read: the largest LDS-resident window, which owns most of its cells
    assert int(pl["ncell"][1]) == M and not pl["home"].any() and int(pl["own"][0]) == M - 199
    pl = check_plan(100000, 409, -1)                          # the longest read whose LDS window owns half of its cells
    assert int(pl["ncell"][1]) == M and not pl["home"].any() and 2 * int(pl["own"][0]) >= M
    pl = check_plan(100000, 410, -1)                          # beyond: SCR_MUL entry positions per sample, rows in device scratch
    assert int(pl["own"][0]) == SCR_MUL * 410 and pl["home"][0] == 1
    pl = check_plan(50000, 2000, -1)
    assert int(pl["own"][0]) == SCR_MUL * 2000 and int(pl["ncell"][1]) == SCR_MUL * 2000 + 3999
    pl = check_plan(100000, 800, 0)
    assert len(pl["first"]) == 1 and pl["home"][0] == 1 and pl["scr_floats"] == 5 * 100000
    assert len(check_plan(3, 800, -1)["first"]) == 1
    P = sa.lib().scrappie_hip_squiggle_local_plan
    assert P(0, 5, -1, 0, None, None, None, None, None, None) == 0
    assert P(5, 0, -1, 0, None, None, None, None, None, None) == 0
    assert P((1 << 30) + 1, 5, -1, 0, None, None, None, None, None, None) == 0


def test_argument_errors_without_gpu():
    """NAN and a text before any GPU work, as squiggle_match_viterbi gives them; the Python layer's own checks"""
    need_feature()
    L = sa.lib()
    params, sig, _ = synth.simulated_squiggle(10, 1)
    good = (1.0, 0.0, 2.0, 5000.0, 5.0)
    PM = C.POINTER(sa._Mat)
    m = oracle.NpMat(params)
    mp = C.cast(m.ptr, PM)
    path = np.zeros(len(sig), dtype=np.int32)
    pp = path.ctypes.data_as(C.POINTER(C.c_int32))

    def rt(start, end, raw=True):
        return sa._RawTable(None, len(sig), start, end, sig.ctypes.data_as(C.POINTER(C.c_float)) if raw else None)

    def both(r, matrix, pens, word):
        s = L.squiggle_match_local_viterbi(r, pens[0], matrix, *pens[1:], pp, None, None)
        assert np.isnan(s) and word in sa.last_error(), (word, sa.last_error())
        s = L.squiggle_match_local_forward(r, pens[0], matrix, *pens[1:])
        assert np.isnan(s) and word in sa.last_error(), (word, sa.last_error())

    both(rt(0, len(sig)), mp, (0.0,) + good[1:], "rate")
    both(rt(0, len(sig)), mp, (1.0, 1.5) + good[2:], "prob_back")
    both(rt(5, 5), mp, good, "empty")
    both(rt(0, len(sig) + 1), mp, good, "past")
    both(rt(0, len(sig), raw=False), mp, good, "signal")
    both(rt(0, len(sig)), None, good, "squiggle")
    empty = sa._Mat(3, 1, 0, 4, m.mat.data)
    both(rt(0, len(sig)), C.pointer(empty), good, "no positions")
    with pytest.raises(ValueError):
        sa.squiggle_match_reference(sa.RawTable(sig), params, viterbi=False, path=True)
    with pytest.raises(TypeError):
        sa.squiggle_match_reference(sig, params)
    with pytest.raises(ValueError):
        sa.squiggle_match_reference(sa.RawTable(sig), params[:, :2])

    class NoEngine(object):
        def __getattr__(self, name):
            raise AssertionError("the argument checks reached the engine (%s)" % name)
    sigs = [np.zeros(100, dtype=np.float32)] * 3
    with pytest.raises(ValueError, match="viterbi"):
        sa.Engine.match_squiggle_reference(NoEngine(), sigs, params, viterbi=False, path=True)
    with pytest.raises(ValueError, match="per signal"):
        sa.Engine.match_squiggle_reference(NoEngine(), sigs, [params, params])
    with pytest.raises(ValueError, match="npos, 3"):
        sa.Engine.match_squiggle_reference(NoEngine(), sigs, params[:, :2])
    with pytest.raises(ValueError, match="per signal"):
        sa.Engine.mappy_reference(NoEngine(), sigs, ["ACGTACGTACGT"] * 2)
    text = open(os.path.join(ROOT, "include", "pyscrap_squiggle.h")).read()
    assert "match_local" not in text                         # the new prototypes are scrappie_hip.h's alone
    assert "squiggle_match_local_viterbi" in open(os.path.join(ROOT, "include", "scrappie_hip.h")).read()


def test_planner_under_sanitizers(tmp_path):
    """tests/squiggle_local_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the planner on arrays of exactly
    as many entries as it says it writes"""
    need_feature()
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "squiggle_local_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "squiggle_local_asan.c"),
                        os.path.join(csrc, "sh_host.c"), "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]
