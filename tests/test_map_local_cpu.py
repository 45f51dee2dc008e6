"""Reads of a transducer model mapped INTO a longer sequence of k-mer states (k_map_local, sh_map_local.h), the part that needs no
GPU: the numpy restatement np_map_local (include/scrappie_hip.h states the definition) with the same cut into windows and the
same order of the end reduction as the kernel, a checker that walks any returned path and re-sums it in float32, the three
arguments that hold the definition, the window planner (scrappie_hip_map_local_plan, csrc/sh_host.c) and tests/map_local_asan.c, a
program of its own over sh_host.c under the address and undefined-behaviour sanitizers.

The definition is map_to_sequence_viterbi / _forward (decode.c:1420-1640, unbanded; np_map in test_map_cpu.py) with the sequence
side made local: the START move at every position, one END accumulator per position.
  * The global paths are a subset and float addition is monotone: local >= global, compared as floats, on every case.
  * One END per position gives the score of one shared END fed by the best position: fl(max(a_i) + b) = max fl(a_i + b).
  * Ownership: a path enters the sequence from START once and advances at most 2 positions per block; window w of stride s owns
    the paths that enter in [w s, (w + 1) s) and holds the cells they can reach; a path's score is the same chain of additions
    wherever it is computed, so the Viterbi score has the same bits for every stride."""
import math
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from test_map_cpu import _lse, np_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1e30
NTH = 256                       # SH_MAP_NTH: threads of a window's workgroup
LDS_BYTES = 65536               # SH_MAP_LDS
WIN_CELLS = 2798                # SH_MAP_LOCAL_CELLS: a window at the default stride, three of them resident per compute unit
WIN_STRIDE = 1200               # SH_MAP_LOCAL_STRIDE: the entry positions it owned where it was measured; never fewer
NR3 = 65                        # states of a k = 3 posterior, stay last
PENS = ((0.0, 0.0, 4.0), (2.0, 0.0, 4.0), (0.0, 2.0, 4.0), (0.0, 0.0, 150.0))
NEW_SYMBOLS = ("map_to_reference_viterbi", "map_to_reference_forward", "scrappie_hip_map_post_local_batch", "scrappie_hip_map_local_plan",
               "scrappie_hip_map_local_stride", "scrappie_hip_map_local_max_cells", "scrappie_hip_map_local_form_counts")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def _r4(n):
    return (n + 3) // 4 * 4


def scr_lds_bytes(nr):
    """the head of 32 words and two columns of the posterior, whole 16-byte pieces"""
    return (32 + 2 * _r4(nr)) * 4


def lds_bytes(ncell, nr):
    """and two score rows, the END row and the codes, each a multiple of 4 entries"""
    return scr_lds_bytes(nr) + 16 * _r4(ncell)


def max_cells(nr):
    return (LDS_BYTES - scr_lds_bytes(nr)) // 16 // 4 * 4


def np_stride(L, nblock, nr, stride):
    """stride > 0: entry positions per window; 0 or None: one window; < 0: the default"""
    reach, M = 2 * (nblock - 1), max_cells(nr)
    if stride is None or stride == 0:
        s = L
    elif stride > 0:
        s = stride
    elif 2 * reach + 1 > M:
        s = 2 * nblock
    elif reach + WIN_STRIDE <= WIN_CELLS <= M:
        s = WIN_CELLS - reach
    else:
        s = M - reach
    return min(max(s, 1), L)


def np_plan(L, nblock, nr, stride):
    """[(first, ncell, own)] per window"""
    s = np_stride(L, nblock, nr, stride)
    return [(c0, min(s + 2 * (nblock - 1), L - c0), min(s, L - c0)) for c0 in range(0, L, s)]


def _reduce(vals, viterbi, dtype):
    """the kernel's end reduction over one row: per thread its cells in order, six butterfly steps in a wave, the waves in order.
    Viterbi: (the first maximum, its index)"""
    n = len(vals)
    if viterbi:
        k = int(np.argmax(vals))
        return vals[k], k
    big = dtype(BIG)
    nch = (n + NTH - 1) // NTH
    pad = np.full(nch * NTH, -big, dtype=dtype)
    pad[:n] = vals
    acc = np.full(NTH, -big, dtype=dtype)
    for ch in range(nch):
        acc = _lse(acc, pad[ch * NTH:(ch + 1) * NTH])
    lane = np.arange(NTH)
    for d in (1, 2, 4, 8, 16, 32):
        acc = _lse(acc, acc[lane ^ d])
    r = acc[0]
    for w in range(1, NTH // 64):
        r = _lse(r, acc[64 * w])
    return r, None


def _window(post, seq, c0, ncell, own, pens, viterbi, dtype, want_tb=False):
    """one window: cells c0 .. c0 + ncell - 1, entry positions c0 .. c0 + own - 1.  Returns (score, end position, ends in E,
    codes, fresh, tie) -- tie: [nblock + 1][ncell] where the one-window run met two equal candidates (the last row: at the end)"""
    f = np.dtype(dtype).type
    NB, nr = post.shape
    big = f(BIG)
    sp, kp, lp_ = f(pens[0]), f(pens[1]), f(pens[2])
    codes_of = np.asarray(seq[c0:c0 + ncell], dtype=np.int64)
    pos = c0 + np.arange(ncell)
    mine = np.arange(ncell) < own
    c = np.full(ncell, -big, dtype=dtype)
    E = np.full(ncell, -big, dtype=dtype)
    start = f(0)
    CODE = np.zeros((NB, ncell), dtype=np.int8) if want_tb else None
    FRESH = np.zeros((NB, ncell), dtype=bool) if want_tb else None
    TIE = np.zeros((NB + 1, ncell), dtype=bool) if want_tb else None
    lb1, lb2 = np.array([-big], dtype=dtype), np.array([-big, -big], dtype=dtype)
    for t in range(NB):
        row = post[t]
        lps = row[nr - 1]
        le = row[codes_of]
        ls = np.fmax(-lp_, lps) if viterbi else _lse(-lp_, lps)
        p = c
        p1 = np.concatenate((lb1, p[:-1]))               # left of the window: no owned path
        p2 = np.concatenate((lb2, p[:-2]))[:ncell]
        v = (p - sp) + lps
        st, sk, fs = p1 + le, (p2 - kp) + le, start + le
        e, ex = E + ls, p - lp_
        if viterbi:
            stay_v = v
            code = np.zeros(ncell, dtype=np.int8)
            m = (pos >= 1) & (st > v)
            v = np.where(m, st, v); code = np.where(m, 1, code)
            m = (pos >= 2) & (sk > v)
            v = np.where(m, sk, v); code = np.where(m, 2, code)
            m = mine & (fs > v)
            v = np.where(m, fs, v); code = np.where(m, 3, code)
            fresh = ex > e
            E = np.where(fresh, ex, e).astype(dtype)
            if want_tb:
                CODE[t], FRESH[t] = code, fresh
                neq = (stay_v == v).astype(int) + ((pos >= 1) & (st == v)) + ((pos >= 2) & (sk == v)) + (mine & (fs == v))
                TIE[t] = ((neq > 1) & (v > -big / 2)) | ((ex == e) & (E > -big / 2))
        else:
            v = np.where(pos >= 1, _lse(v, st), v)
            v = np.where(pos >= 2, _lse(v, sk), v)
            v = np.where(mine, _lse(v, fs), v)
            E = _lse(e, ex).astype(dtype)
        c = v.astype(dtype)
        start = f(start + ls)
    x, kx = _reduce(c, viterbi, dtype)
    y, ky = _reduce(E, viterbi, dtype)
    if not viterbi:
        return _lse(x, y), None, None, None, None, None
    in_e = not (x > y)
    k = ky if in_e else kx
    if want_tb:
        TIE[NB, k] = (x == y) or int(((E if in_e else c) == (y if in_e else x)).sum()) > 1
    return np.fmax(x, y), c0 + k, in_e, CODE, FRESH, TIE


def np_map_local(post, seq, stay_pen=0.0, skip_pen=0.0, local_pen=4.0, stride=None, viterbi=True, dtype=np.float32, info=None):
    """The specification.  post [nblock][nr] log-posterior, stay last; seq: L state codes.  The positions are cut into windows of
    `stride` entry positions each (None or 0: one window; -1: the default), each computed alone; the highest window, the lowest
    on a tie -- forward: _lse over the windows in their order.  Returns (score, first, last, path): path[blk] the position or -1
    in START / END, first the lowest position visited and last the highest plus one; forward: (score, None, None, None).
    info (a dict): 'tie_free' -- no two equal candidates met anywhere on the path of this run."""
    post = np.ascontiguousarray(post, dtype=dtype)
    seq = np.asarray(seq, dtype=np.int64)
    NB, nr = post.shape
    L = len(seq)
    assert NB >= 1 and L >= 1 and nr >= 2
    pens = (stay_pen, skip_pen, local_pen)
    plan = np_plan(L, NB, nr, stride)
    res = [_window(post, seq, c0, nc, own, pens, viterbi, dtype) for c0, nc, own in plan]
    if not viterbi:
        acc = res[0][0]
        for r in res[1:]:
            acc = _lse(acc, r[0])
        return acc, None, None, None
    scores = np.array([r[0] for r in res], dtype=dtype)
    w = int(np.argmax(scores))
    c0, nc, own = plan[w]
    score, pe, in_e, CODE, FRESH, TIE = _window(post, seq, c0, nc, own, pens, True, dtype, want_tb=True)
    assert np.asarray(score).tobytes() == np.asarray(res[w][0]).tobytes() and (pe, in_e) == (res[w][1], res[w][2])
    path = np.full(NB, -1, dtype=np.int32)
    j, st = pe - c0, (1 if in_e else 0)                  # 0: the cell j, 1: its E, 2: START
    tie = bool(TIE[NB, j]) or int((scores == scores[w]).sum()) > 1
    for blk in range(NB - 1, -1, -1):
        if st == 0:
            path[blk] = c0 + j
        if st != 2:
            tie = tie or bool(TIE[blk, j])
        if st == 1:
            if FRESH[blk, j]:
                st = 0
        elif st == 0:
            if CODE[blk, j] == 3:
                st = 2
            else:
                j -= int(CODE[blk, j])
                assert j >= 0
    assert st == 2
    on = path[path >= 0]
    assert len(on) >= 1 and c0 <= on[0] < c0 + own
    if info is not None:
        info["tie_free"] = not tie
    return score, int(on.min()), int(on.max()) + 1, path


def check_local_path(post, seq, pens, score, first, last, path):
    """the path is admissible -- START, then positions that advance by 0, 1 or 2, then END --, visits first .. last - 1, and its
    sequential float32 sum is the score in bits"""
    f = np.float32
    post = np.ascontiguousarray(post, dtype=np.float32)
    NB, nr = post.shape
    L = len(seq)
    path = np.asarray(path, dtype=np.int64)
    sp, kp, lp_ = f(pens[0]), f(pens[1]), f(pens[2])
    assert len(path) == NB
    on = np.nonzero(path >= 0)[0]
    assert len(on) >= 1 and np.array_equal(on, np.arange(on[0], on[-1] + 1))
    assert 0 <= first < last <= L and path[on[0]] == first and path[on[-1]] == last - 1
    total = f(0)
    for t in range(NB):
        row = post[t]
        lps = row[nr - 1]
        ls = np.fmax(-lp_, lps)
        if t < on[0] or t > on[-1] + 1:
            total = f(total + ls)                        # START -> START, END -> END
        elif t == on[-1] + 1:
            total = f(total - lp_)                       # the sequence -> END
        elif t == on[0]:
            total = f(total + row[seq[path[t]]])         # START -> the sequence
        else:
            d = path[t] - path[t - 1]
            assert d in (0, 1, 2)
            if d == 0:
                total = f(f(total - sp) + lps)
            elif d == 1:
                total = f(total + row[seq[path[t]]])
            else:
                total = f(f(total - kp) + row[seq[path[t]]])
    assert total.tobytes() == np.float32(score).tobytes(), (total, score)


def rand_post(nblock, nr, rng, scale=3.0):
    """a random log-posterior: log-softmax of scaled normals, float32"""
    z = scale * rng.standard_normal((nblock, nr))
    z -= z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)


def planted(ref, a, b, nr, lead=0, trail=0, p=0.9):
    """log p on the states of a path that waits `lead` blocks in START, steps once per block through ref[a:b), then waits `trail`
    blocks in END; the rest spread evenly.  The blocks in START and END are flat, log(1 / nr) = -4.17 for 65 states: below the
    local penalty of 4 that START and END pay per block, so waiting there beats any state of the sequence"""
    nb = lead + (b - a) + trail
    post = np.full((nb, nr), np.log(1.0 / nr), dtype=np.float32)
    want = np.full(nb, -1, dtype=np.int32)
    for t in range(lead, lead + (b - a)):
        post[t, :] = np.float32(np.log((1 - p) / (nr - 1)))
        post[t, ref[a + t - lead]] = np.float32(np.log(p))
        want[t] = a + t - lead
    return post, want


def local_cases():
    """(name, post, seq) at L = nblock scale: random float posteriors, k = 3"""
    rng = np.random.default_rng(2024)
    out = []
    for i, (nb, L) in enumerate(((1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (1, 7), (5, 5), (9, 20), (20, 9), (30, 30), (17, 64), (64, 17), (40, 90),
                                 (65, 65), (33, 200), (12, 300), (70, 40), (25, 26), (8, 3), (3, 8))):
        out.append(("rand-%d-%dx%d" % (i, nb, L), rand_post(nb, NR3, rng), rng.integers(0, NR3 - 1, L).astype(np.int32)))
    return out


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    for name in NEW_SYMBOLS:
        assert hasattr(sa.lib(), name), name
    assert set(sa.map_local_form_counts()) == {(v, t, s) for v in (False, True) for t in (False, True) for s in (False, True)}
    for nr in (5, 17, 65, 257, 1025):
        assert sa.map_local_max_cells(nr) == max_cells(nr)
        assert lds_bytes(max_cells(nr), nr) <= LDS_BYTES < lds_bytes(max_cells(nr) + 1, nr)
    assert max_cells(1025) == 3572 and max_cells(65) == 4052
    assert set(sa.map_crf_local_form_counts()) == {(v, t, s) for v in (False, True) for t in (False, True) for s in (False, True)}      # the CRF family's own, as before


def test_local_is_never_below_global():
    """the global paths are a subset: Viterbi local >= map_to_sequence_viterbi restated, as floats, on every case and penalty set"""
    n = 0
    for name, post, seq in local_cases():
        for pens in PENS:
            g = np_map(post, seq, *pens, viterbi=True)[0]
            s, first, last, path = np_map_local(post, seq, *pens)
            check_local_path(post, seq, pens, s, first, last, path)
            assert np.float32(s) >= np.float32(g), (name, pens, s, g)
            n += 1
    assert n == 80


def test_one_end_per_position_is_one_shared_end():
    """fl(max(a_i) + b) = max fl(a_i + b): a single END fed by the best position each block gives the score's bits"""
    f = np.float32
    for name, post, seq in local_cases():
        for pens in PENS:
            sp, kp, lp_ = (f(v) for v in pens)
            NB, nr = post.shape
            L = len(seq)
            c = np.full(L, -f(BIG), dtype=np.float32)
            end, start = -f(BIG), f(0)
            for t in range(NB):
                row = post[t]
                lps, le = row[nr - 1], row[seq]
                ls = np.fmax(-lp_, lps)
                p1 = np.concatenate(([-f(BIG)], c[:-1])).astype(np.float32)
                p2 = np.concatenate(([-f(BIG)] * 2, c[:-2]))[:L].astype(np.float32)
                v = (c - sp) + lps
                v = np.fmax(v, np.where(np.arange(L) >= 1, p1 + le, -f(BIG)))
                v = np.fmax(v, np.where(np.arange(L) >= 2, (p2 - kp) + le, -f(BIG)))
                v = np.fmax(v, start + le)
                end = np.fmax(f(end + ls), f(c.max() - lp_))
                c, start = v.astype(np.float32), f(start + ls)
            want = np.fmax(c.max(), end)
            got = np_map_local(post, seq, *pens)[0]
            assert np.float32(got).tobytes() == np.float32(want).tobytes(), (name, pens)


@pytest.mark.parametrize("flank", (0, 1, 37))
def test_planted_paths_are_found(flank):
    """log 0.9 along a path that steps once per block through ref[a:b) inside random flanks: exactly (a, b) and the planted path;
    with blocks of START before and END behind: a path that ends in END from an interior position"""
    n = 0
    for seed in range(6):
        rng = np.random.default_rng(1000 + 10 * flank + seed)
        core = 12 + 5 * seed
        ref = rng.integers(0, NR3 - 1, flank + core + flank).astype(np.int32)
        a, b = flank, flank + core
        for lead, trail in ((0, 0), (3, 0), (0, 4), (2, 2)):
            post, want = planted(ref, a, b, NR3, lead, trail)
            for stride in (None, 7, -1):
                s, first, last, path = np_map_local(post, ref, 0.0, 0.0, 4.0, stride=stride)
                assert (first, last) == (a, b), (flank, seed, lead, trail, stride, first, last)
                assert np.array_equal(path, want), (flank, seed, lead, trail, stride)
                check_local_path(post, ref, (0.0, 0.0, 4.0), s, first, last, path)
                assert (path[-1] == -1) == (trail > 0)           # ends in END from position b - 1 < L - 1 where flank > 0; else in the sequence
                n += 1
    assert n == 72


def test_every_stride_gives_the_one_window_bits():
    """strides 1, 7, 64, the default and one window: the score in bits; the path wherever the one-window run met no tie, which
    random float posteriors give on at least 90 % of the cases"""
    n = free = 0
    for name, post, seq in local_cases():
        for pens in PENS:
            info = {}
            s0, f0, l0, p0 = np_map_local(post, seq, *pens, info=info)
            n += 1
            free += info["tie_free"]
            for stride in (1, 7, 64, -1, len(seq)):
                s, f, l, p = np_map_local(post, seq, *pens, stride=stride)
                assert np.float32(s).tobytes() == np.float32(s0).tobytes(), (name, pens, stride)
                check_local_path(post, seq, pens, s, f, l, p)
                if info["tie_free"]:
                    assert (f, l) == (f0, l0) and np.array_equal(p, p0), (name, pens, stride)
    print("tie-free cases: %d of %d" % (free, n))
    assert n == 80 and free >= 0.9 * n


def _count_paths(NB, L):
    """state sequences START -> ... over NB blocks that end in a cell or an E: START and END repeat in two ways per block (stay, or
    the local penalty's move), a cell stays, steps or skips or leaves for its E, START enters at any position"""
    start, cell, end = 1, [0] * L, [0] * L
    for _ in range(NB):
        ncell = [cell[i] + (cell[i - 1] if i >= 1 else 0) + (cell[i - 2] if i >= 2 else 0) + start for i in range(L)]
        end = [2 * end[i] + cell[i] for i in range(L)]
        start, cell = 2 * start, ncell
    return sum(cell) + sum(end)


def test_forward_windows_partition_the_paths():
    """float64: the windows' forward scores sum to the one window's -- ownership is a partition; an all-zero posterior with no
    penalties: every path scores 0, so the forward score is the log of their number"""
    rng = np.random.default_rng(5)
    for NB, L in ((1, 1), (3, 2), (7, 30), (20, 7), (17, 64)):
        post = rand_post(NB, NR3, rng).astype(np.float64)
        seq = rng.integers(0, NR3 - 1, L)
        for pens in PENS[:3]:
            one = np_map_local(post, seq, *pens, viterbi=False, dtype=np.float64)[0]
            for stride in (1, 3, 7, -1, L):
                got = np_map_local(post, seq, *pens, stride=stride, viterbi=False, dtype=np.float64)[0]
                assert abs(float(got) - float(one)) <= 1e-10 * max(1.0, abs(float(one))), (NB, L, pens, stride)
    for NB in range(1, 7):
        for L in range(1, 9):
            z = np.zeros((NB, NR3))
            seq = rng.integers(0, NR3 - 1, L)
            for stride in (None, 3):
                got = np_map_local(z, seq, 0.0, 0.0, 0.0, stride=stride, viterbi=False, dtype=np.float64)[0]
                assert abs(float(got) - math.log(_count_paths(NB, L))) < 1e-9, (NB, L, stride)


def test_smallest_shapes():
    """nblock = 1: the path is one START move, the best single entry; L = 1 and L = 2: pos 0 has no step, pos 1 no skip"""
    rng = np.random.default_rng(11)
    for L in (1, 2, 3, 9):
        post = rand_post(1, NR3, rng)
        seq = rng.permutation(NR3 - 1)[:L].astype(np.int32)
        s, first, last, path = np_map_local(post, seq)
        k = int(np.argmax(post[0, seq]))
        assert np.float32(s).tobytes() == np.float32(post[0, seq[k]]).tobytes() and (first, last) == (k, k + 1) and path.tolist() == [k]
    for L in (1, 2):
        for NB in (2, 3, 6):
            post = rand_post(NB, NR3, rng)
            seq = rng.integers(0, NR3 - 1, L).astype(np.int32)
            for pens in PENS:
                s, first, last, path = np_map_local(post, seq, *pens)
                check_local_path(post, seq, pens, s, first, last, path)
                assert np.float32(s) >= np.float32(np_map(post, seq, *pens, viterbi=True)[0])
                assert 0 <= first < last <= L and np.all(np.diff(path[path >= 0]) <= 1)       # two positions: never a skip
    # a path that ends in the sequence, and one that leaves an interior position for END
    ref = np.arange(10, 30).astype(np.int32)
    post, want = planted(ref, 4, 12, NR3)
    s, first, last, path = np_map_local(post, ref)
    assert (first, last) == (4, 12) and path[-1] == 11 and np.array_equal(path, want)
    post, want = planted(ref, 4, 12, NR3, trail=5)
    s, first, last, path = np_map_local(post, ref)
    assert (first, last) == (4, 12) and path[-6:].tolist() == [11, -1, -1, -1, -1, -1] and np.array_equal(path, want)


def check_plan(L, nblock, nr, stride):
    pl = sa.map_local_plan(L, nblock, nr, stride)
    s = int(sa.lib().scrappie_hip_map_local_stride(L, nblock, nr, stride))
    assert s == np_stride(L, nblock, nr, stride), (L, nblock, nr, stride)
    want = np_plan(L, nblock, nr, stride)
    nw = len(pl["first"])
    assert nw == len(want) and nw >= 1
    at = 0
    for w in range(nw):
        first, ncell, own = int(pl["first"][w]), int(pl["ncell"][w]), int(pl["own"][w])
        assert (first, ncell, own) == want[w], (L, nblock, nr, stride, w)
        assert first == at and own >= 1                      # every entry position 0 .. L - 1 is owned exactly once
        at += own
        assert first + ncell - 1 == min(first + s - 1 + 2 * (nblock - 1), L - 1)
        assert ncell >= own
        assert int(pl["home"][w]) == (1 if lds_bytes(ncell, nr) > LDS_BYTES else 0), (L, nblock, nr, stride, w)
    assert at == L
    end = 0
    for w in range(nw):
        off = int(pl["scr_off"][w])
        if not pl["home"][w]:
            assert off == -1
            continue
        assert off % 4 == 0 and off >= end, (L, nblock, nr, stride, w)          # 16-byte aligned, disjoint
        end = off + 3 * _r4(int(pl["ncell"][w]))
    assert pl["scr_floats"] == end
    return pl


def test_planner():
    for nr in (65, 1025):
        M = max_cells(nr)
        for L in (1, 2, 5, 63, 64, 300, 5000, 3 * M + 11):
            for nblock in (1, 2, 7, 64, 800, 801, M // 4, M // 4 + 1, M // 4 + 2, M + 40):
                for stride in (1, 7, 64, L + 5, 0, -1, 3000, M, M + 1):
                    if stride == 1 and L > 300:
                        continue
                    check_plan(L, nblock, nr, stride)
    M = max_cells(1025)
    pl = check_plan(100000, 800, 1025, -1)                   # the default as measured: a window of 2798 cells, three resident per compute unit, stride 1200
    assert int(pl["ncell"][0]) == WIN_CELLS and not pl["home"].any() and int(pl["own"][0]) == WIN_STRIDE == WIN_CELLS - 1598
    assert lds_bytes(WIN_CELLS, 1025) * 3 <= 160 * 1024 < lds_bytes(WIN_CELLS, 1025) * 4
    pl = check_plan(100000, 200, 1025, -1)                   # a shorter read: the same window owns more of its cells
    assert int(pl["ncell"][0]) == WIN_CELLS and not pl["home"].any() and int(pl["own"][0]) == WIN_CELLS - 398
    pl = check_plan(100000, 801, 1025, -1)                   # a longer one would own fewer than it was measured with: the largest LDS-resident window
    assert int(pl["ncell"][0]) == M and not pl["home"].any() and int(pl["own"][0]) == M - 1600
    pl = check_plan(100000, M // 4, 1025, -1)                # the longest read whose window owns more than half of its cells in LDS
    assert int(pl["ncell"][0]) == M and not pl["home"].any() and 2 * int(pl["own"][0]) > M
    pl = check_plan(100000, 8000, 1025, -1)                  # a window that owns half of its cells exceeds LDS: stride 2 nblock, in scratch
    assert int(pl["own"][0]) == 16000 and pl["home"][0] == 1
    pl = check_plan(100000, 800, 1025, 0)
    assert len(pl["first"]) == 1 and pl["home"][0] == 1 and pl["scr_floats"] == 3 * 100000
    assert len(check_plan(3, 800, 1025, -1)["first"]) == 1   # L < nblock: one window holds everything
    P = sa.lib().scrappie_hip_map_local_plan
    assert P(0, 5, 65, -1, 0, None, None, None, None, None, None) == 0
    assert P(5, 0, 65, -1, 0, None, None, None, None, None, None) == 0
    assert P(5, 5, 1, -1, 0, None, None, None, None, None, None) == 0
    assert P((1 << 30) + 1, 5, 65, -1, 0, None, None, None, None, None, None) == 0


def test_python_argument_checks():
    m = sa.ScrappyMatrix.from_numpy(np.zeros((4, NR3), dtype=np.float32), sloika=False)
    with pytest.raises(ValueError):
        sa.map_post_to_reference(m, "ACGTACGT", viterbi=False, path=True)
    with pytest.raises(TypeError):
        sa.map_post_to_reference(np.zeros((4, NR3), dtype=np.float32), "ACGTACGT")
    with pytest.raises(ValueError):
        sa.map_post_to_reference(m, "ACNTT")

    class NoEngine(object):
        def __getattr__(self, name):
            raise AssertionError("the argument checks reached the engine (%s)" % name)
    sigs = [np.zeros(1000, dtype=np.float32)] * 3
    with pytest.raises(ValueError, match="viterbi"):
        sa.Engine.map_to_reference_transducer(NoEngine(), sigs, "ACGTACGT", viterbi=False, path=True)
    with pytest.raises(ValueError, match="per signal"):
        sa.Engine.map_to_reference_transducer(NoEngine(), sigs, ["ACGTACGT", "ACGTACGT"])


def test_planner_under_sanitizers(tmp_path):
    """tests/map_local_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the planner on arrays of exactly
    as many entries as it says it writes"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "map_local_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "map_local_asan.c"),
                        os.path.join(csrc, "sh_host.c"), "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]
