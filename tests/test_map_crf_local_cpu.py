"""Reads of a flip-flop (CRF) model mapped INTO a longer base sequence (k_map_crf_local, sh_map_crf_local.h), the part that needs
no GPU: the numpy restatement (np_map_crf_local: include/scrappie_hip.h states it) with the same cut into windows and the same
order of the end reduction as the kernel, a checker of local paths, the identities that hold the definition against decode_crf
restated (np_decode_crf, test_map_crf_cpu.py), the window planner (scrappie_hip_map_crf_local_plan, csrc/sh_host.c) and
tests/map_crf_local_asan.c, a program of its own over sh_host.c under the address and undefined-behaviour sanitizers.

The pins need no tolerance.  Float addition is monotone, the local paths are a subset of decode_crf's and contain decode_crf's own
path whenever the read's call occurs in the sequence: mapping a read into flank + call + flank returns decode_crf's score in bits.
A window owns the paths that start in its stride of cells, every path lies wholly inside the window that owns it, and a path's
score is the same chain of additions wherever it is computed: the Viterbi score has the same bits for every stride."""
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from test_map_crf_cpu import _lse, _trans, map_crf_cases, np_decode_crf, np_map_crf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1e30
NTH = 256                       # SH_MAP_NTH: threads of a window's workgroup
LDS_BYTES = 65536               # SH_MAP_LDS
WIN_CELLS = 2034                # SH_MAP_CRF_LOCAL_CELLS: a window at the default stride, four of them resident per compute unit
NEW_SYMBOLS = ("map_crf_to_reference_viterbi", "map_crf_to_reference_forward", "scrappie_hip_map_local_batch",
               "scrappie_hip_free_map_local_results", "scrappie_hip_map_crf_local_plan", "scrappie_hip_map_crf_local_stride",
               "scrappie_hip_map_crf_local_max_cells", "scrappie_hip_map_crf_local_form_counts")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def lds_bytes(ncell):
    """two columns of 32 transitions, four rows of ncell + 1 floats, ncell codes"""
    return (64 + 4 * (ncell + 1) + ncell) * 4


def max_cells():
    return (LDS_BYTES - lds_bytes(0)) // (lds_bytes(1) - lds_bytes(0))


def np_stride(L, nblock, stride):
    """stride > 0: cells; 0 or None: one window; < 0: the default"""
    if stride is None or stride == 0:
        s = L + 1
    elif stride > 0:
        s = stride
    elif nblock + 1 > max_cells():
        s = nblock
    elif 2 * nblock <= WIN_CELLS <= max_cells():
        s = WIN_CELLS - nblock
    else:
        s = max_cells() - nblock
    return min(max(s, 1), L + 1)


def np_plan(L, nblock, stride):
    """[(first, ncell, own)] per window"""
    s = np_stride(L, nblock, stride)
    out = []
    for c0 in range(0, L + 1, s):
        last = min(c0 + s - 1 + nblock, L)
        out.append((c0, last - c0 + 1, min(s, L + 1 - c0)))
    return out


def _window(tr_all, seq, c0, ncell, own, viterbi, dtype, want_tb=False):
    """one window: cells c0 .. c0 + ncell - 1, start cells c0 .. c0 + own - 1.  Returns (score, end p, end kind, KB, KS)"""
    NB, L = tr_all.shape[0], len(seq)
    big = dtype(BIG)
    p = c0 + np.arange(ncell)
    b = seq[np.clip(p - 1, 0, L - 1)]
    bp = seq[np.clip(p - 2, 0, L - 1)]
    iBB, iBS, iSB = 5 * b + bp, 5 * b + 4, 20 + b
    mine = np.arange(ncell) < own
    B = np.where(mine & (p >= 1), dtype(0), -big).astype(dtype)
    S = np.where(mine, dtype(0), -big).astype(dtype)
    KB = np.zeros((NB, ncell), dtype=bool) if want_tb else None
    KS = np.zeros((NB, ncell), dtype=bool) if want_tb else None
    left = np.array([-big], dtype=dtype)
    with np.errstate(over="ignore"):
        for t in range(NB):
            tr = tr_all[t]
            B1 = np.concatenate((left, B[:-1]))              # left of the window: no owned path
            S1 = np.concatenate((left, S[:-1]))
            bb, bs = tr[iBB] + B1, tr[iBS] + S1
            sb, ss = tr[iSB] + B, tr[24] + S
            if viterbi:
                kb = (p < 2) | (bs > bb)
                ks = (p < 1) | (ss > sb)
                nB, nS = np.where(kb, bs, bb), np.where(ks, ss, sb)
                if want_tb:
                    KB[t], KS[t] = kb, ks
            else:
                nB = np.where(p < 2, bs, _lse(bb, bs))
                nS = np.where(p < 1, ss, _lse(sb, ss))
            nB = np.where(p < 1, -big, nB)                   # there is no B[0]
            B, S = nB.astype(dtype), nS.astype(dtype)
        if viterbi:
            both = np.empty(2 * ncell, dtype=dtype)          # the scan: p ascending, B[p] before S[p]; the first maximum
            both[0::2], both[1::2] = B, S
            k = int(np.argmax(both))
            return both[k], c0 + k // 2, k % 2, KB, KS
        # forward: per thread its cells in order (sh_lse(-big, x) is x), six butterfly steps in a wave, the waves in order
        nch = (ncell + NTH - 1) // NTH
        pb = np.full(nch * NTH, -big, dtype=dtype)
        ps = pb.copy()
        pb[:ncell], ps[:ncell] = B, S
        acc = np.full(NTH, -big, dtype=dtype)
        for ch in range(nch):
            acc = _lse(acc, pb[ch * NTH:(ch + 1) * NTH])
            acc = _lse(acc, ps[ch * NTH:(ch + 1) * NTH])
        lane = np.arange(NTH)
        for d in (1, 2, 4, 8, 16, 32):
            acc = _lse(acc, acc[lane ^ d])
        r = acc[0]
        for w in range(1, NTH // 64):
            r = _lse(r, acc[64 * w])
        return r, None, None, None, None


def np_map_crf_local(trans, seq, stride=None, viterbi=True, dtype=np.float32):
    """The specification.  trans [nblock][25], seq: L bases coded 0..3; cells and the block recursion as np_map_crf.  Entry 0:
    S[p] = 0 for p = 0 .. L, B[p] = 0 for p = 1 .. L; the end: the first maximum over all cells of entry nblock, p ascending and
    B[p] before S[p]; forward: _lse over them.  The cells are cut into windows of `stride` start cells each (None or 0: one
    window; -1: the default), each computed alone; the highest window, the lowest on a tie -- forward: _lse over the windows in
    their order.  Returns (score, first, last, path): the read spells seq[first:last], path[t] is the index of the last base
    emitted through entry t, first - 1 while none; forward: (score, None, None, None)."""
    tr_all = np.ascontiguousarray(trans, dtype=dtype)
    seq = np.asarray(seq, dtype=np.int64)
    NB, L = tr_all.shape[0], len(seq)
    assert tr_all.shape[1] == 25 and NB >= 1 and L >= 1
    plan = np_plan(L, NB, stride)
    res = [_window(tr_all, seq, c0, nc, own, viterbi, dtype) for c0, nc, own in plan]
    if not viterbi:
        acc = res[0][0]
        for r in res[1:]:
            acc = _lse(acc, r[0])
        return acc, None, None, None
    w = int(np.argmax(np.array([r[0] for r in res], dtype=dtype)))
    c0, nc, own = plan[w]
    score, pe, kind, KB, KS = _window(tr_all, seq, c0, nc, own, True, dtype, want_tb=True)
    assert np.asarray(score).tobytes() == np.asarray(res[w][0]).tobytes()
    path = np.zeros(NB + 1, dtype=np.int32)
    p = pe
    for t in range(NB, 0, -1):
        path[t] = p - 1
        stay = (KS if kind else KB)[t - 1, p - c0]
        if kind == 0:
            p -= 1
        kind = 1 if stay else 0
    path[0] = p - 1
    assert c0 <= p < c0 + own
    return score, p - (1 if kind == 0 else 0), pe, path


def check_local_path(trans, seq, score, first, last, path):
    """the path is admissible, spells seq[first:last], and its sequential float32 sum is the score in bits"""
    trans = np.ascontiguousarray(trans, dtype=np.float32)
    NB, L = trans.shape[0], len(seq)
    path = np.asarray(path, dtype=np.int64)
    assert len(path) == NB + 1
    assert 0 <= first <= last <= L
    assert path[0] in (first - 1, first) and path[NB] == last - 1
    step = np.diff(path)
    assert np.all((step == 0) | (step == 1))
    base = np.concatenate(([path[0] == first], step == 1))
    assert int(base.sum()) == last - first                  # the base entries, in order, are seq[first:last]
    state = np.where(base, np.asarray(seq)[np.clip(path, 0, L - 1)], 4)
    total = np.float32(0)
    for t in range(NB):
        total = np.float32(trans[t, 5 * state[t + 1] + state[t]] + total)
    assert total.tobytes() == np.float32(score).tobytes(), (total, score)


def local_cases():
    """map_crf_cases() that have an admissible global path or not: every one has a local one"""
    return map_crf_cases()


def embed(c, nl, nr, rng):
    """flank + the case's call + flank, and where the call first occurs in it"""
    left, right = rng.integers(0, 4, nl), rng.integers(0, 4, nr)
    ref = np.concatenate((left, c["seq"], right)).astype(np.int32)
    s, call = "".join("ACGT"[b] for b in ref), "".join("ACGT"[b] for b in c["seq"])
    return ref, s.find(call)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    for name in NEW_SYMBOLS:
        assert hasattr(sa.lib(), name), name
    assert set(sa.map_crf_local_form_counts()) == {(v, t, s) for v in (False, True) for t in (False, True) for s in (False, True)}
    assert sa.map_crf_local_max_cells() == max_cells() == (65536 - 4 * 68) // 20
    assert set(sa.map_crf_form_counts()) == {(v, t, s) for v in (False, True) for t in (False, True) for s in (False, True)}      # the global kernel's own, as before


def test_embedding_identity_against_decode_crf():
    """flank + call + flank: decode_crf's score in bits, first, last and the shifted path"""
    rng = np.random.default_rng(101)
    n = 0
    for c in local_cases():
        if not c["from_call"]:
            continue
        ds, dp = np_decode_crf(c["trans"])
        assert np.float32(ds).tobytes() == np.float32(c["dscore"]).tobytes()
        for nl, nr in ((0, 0), (1, 0), (0, 1), (1, 1), (37, 0), (0, 37), (37, 37), (1, 37)):
            if c["trans"].shape[0] > 200 and (nl, nr) not in ((0, 0), (37, 37)):
                continue
            ref, at = embed(c, nl, nr, rng)
            s, first, last, path = np_map_crf_local(c["trans"], ref)
            assert np.float32(s).tobytes() == np.float32(ds).tobytes(), (c["name"], nl, nr, s, ds)
            assert (first, last) == (at, at + len(c["seq"])), (c["name"], nl, nr, first, last, at)
            assert np.array_equal(path, c["dpath"] + at), (c["name"], nl, nr)
            check_local_path(c["trans"], ref, s, first, last, path)
            n += 1
    assert n >= 100


def test_local_is_never_below_global():
    n = 0
    for c in local_cases():
        g = np_map_crf(c["trans"], c["seq"])[0]
        s, first, last, path = np_map_crf_local(c["trans"], c["seq"])
        check_local_path(c["trans"], c["seq"], s, first, last, path)
        if np.isnan(g):
            continue                                    # no global path: there is always a local one
        assert np.float32(s) >= np.float32(g), c["name"]
        n += 1
    assert n >= 30


def test_every_stride_gives_the_one_window_bits():
    """strides 1, 7, 64 and L + 1 against one window: the score in bits, and on these continuous data first, last and the path"""
    n = 0
    for c in local_cases():
        NB, L = c["trans"].shape
        L = len(c["seq"])
        tie = c["name"].startswith("all-zero")
        s0, f0, l0, p0 = np_map_crf_local(c["trans"], c["seq"])
        for stride in (1, 7, 64, L + 1):
            if NB * ((L + stride) // stride) > 6000:
                continue
            s, f, l, p = np_map_crf_local(c["trans"], c["seq"], stride=stride)
            assert np.float32(s).tobytes() == np.float32(s0).tobytes(), (c["name"], stride)
            check_local_path(c["trans"], c["seq"], s, f, l, p)
            if not tie:
                assert (f, l) == (f0, l0) and np.array_equal(p, p0), (c["name"], stride)
            n += 1
    assert n >= 60


def test_forward_windows_partition_the_paths():
    """float64: the windows' forward scores sum to the one window's -- ownership is a partition; all-zero: every path scores 0, so
    the forward score is the log of their number, sum over start cells and lengths of C(nblock + [start is S], bases)"""
    import math
    rng = np.random.default_rng(5)
    for NB, L in ((1, 1), (3, 2), (7, 30), (20, 7), (17, 64)):
        tr = _trans(NB, 2.0, rng)
        seq = rng.integers(0, 4, L)
        one = np_map_crf_local(tr, seq, viterbi=False, dtype=np.float64)[0]
        for stride in (1, 3, 7, L + 1):
            got = np_map_crf_local(tr, seq, stride=stride, viterbi=False, dtype=np.float64)[0]
            assert abs(float(got) - float(one)) <= 1e-10 * max(1.0, abs(float(one))), (NB, L, stride)
        z = np.zeros((NB, 25))
        count = 0
        for p0 in range(L + 1):                         # start in S[p0]: any k <= L - p0 of the NB later entries are bases
            count += sum(math.comb(NB, k) for k in range(0, min(NB, L - p0) + 1))
        for p0 in range(1, L + 1):                      # start in B[p0]
            count += sum(math.comb(NB, k) for k in range(0, min(NB, L - p0) + 1))
        got = np_map_crf_local(z, seq, stride=3, viterbi=False, dtype=np.float64)[0]
        assert abs(float(got) - math.log(count)) < 1e-9, (NB, L)


def test_tie_cases_pass_the_checker():
    rng = np.random.default_rng(9)
    for tr, seq in ((_trans(40, 2.0, rng), [2] * 90), (np.zeros((12, 25), dtype=np.float32), rng.integers(0, 4, 40)),
                    (np.zeros((9, 25), dtype=np.float32), [1] * 5)):
        s0 = None
        for stride in (None, 1, 7):
            s, f, l, p = np_map_crf_local(tr, seq, stride=stride)
            check_local_path(tr, np.asarray(seq), s, f, l, p)
            s0 = s if s0 is None else s0
            assert np.float32(s).tobytes() == np.float32(s0).tobytes()


def check_plan(L, nblock, stride):
    pl = sa.map_crf_local_plan(L, nblock, stride)
    s = int(sa.lib().scrappie_hip_map_crf_local_stride(L, nblock, stride))
    assert s == np_stride(L, nblock, stride), (L, nblock, stride)
    want = np_plan(L, nblock, stride)
    nw = len(pl["first"])
    assert nw == len(want) and nw >= 1
    at = 0
    for w in range(nw):
        first, ncell, own = int(pl["first"][w]), int(pl["ncell"][w]), int(pl["own"][w])
        assert (first, ncell, own) == want[w], (L, nblock, stride, w)
        assert first == at and own >= 1                      # every start cell 0 .. L is owned exactly once
        at += own
        assert first + ncell - 1 == min(first + s - 1 + nblock, L)
        assert ncell >= own
        assert int(pl["home"][w]) == (1 if lds_bytes(ncell) > LDS_BYTES else 0), (L, nblock, stride, w)
    assert at == L + 1
    end = 0
    for w in range(nw):
        off = int(pl["scr_off"][w])
        if not pl["home"][w]:
            assert off == -1
            continue
        assert off % 4 == 0 and off >= end, (L, nblock, stride, w)          # 16-byte aligned, disjoint
        end = off + 4 * (int(pl["ncell"][w]) + 1)
    assert pl["scr_floats"] == end
    return pl


def test_planner():
    M = max_cells()
    for L in (1, 2, 5, 63, 64, 300, 5000, 3 * M + 11):
        for nblock in (1, 2, 7, 64, 800, M - 1, M, M + 40):
            for stride in (1, 7, 64, L + 5, 0, -1, 3000, M, M + 1):
                if stride == 1 and L > 300:
                    continue
                check_plan(L, nblock, stride)
    pl = check_plan(100000, 800, -1)                         # the default: a window of 2034 cells, four resident per compute unit
    assert int(pl["ncell"][0]) == WIN_CELLS and not pl["home"].any() and int(pl["own"][0]) == WIN_CELLS - 800
    assert lds_bytes(WIN_CELLS) * 4 <= 160 * 1024 < lds_bytes(WIN_CELLS + 1) * 4
    pl = check_plan(100000, 1400, -1)                        # less than half of such a window would be owned: the largest LDS-resident one
    assert int(pl["ncell"][0]) == M and not pl["home"].any() and int(pl["own"][0]) == M - 1400
    pl = check_plan(100000, M + 40, -1)                      # nblock + 1 cells alone exceed it: stride nblock, in scratch
    assert int(pl["own"][0]) == M + 40 and pl["home"][0] == 1
    pl = check_plan(100000, 800, 0)
    assert len(pl["first"]) == 1 and pl["home"][0] == 1 and pl["scr_floats"] == 4 * 100002
    assert len(check_plan(3, 800, -1)["first"]) == 1         # L < nblock: one window holds everything
    assert sa.lib().scrappie_hip_map_crf_local_plan(0, 5, -1, 0, None, None, None, None, None, None) == 0
    assert sa.lib().scrappie_hip_map_crf_local_plan(5, 0, -1, 0, None, None, None, None, None, None) == 0
    assert sa.lib().scrappie_hip_map_crf_local_plan((1 << 30) + 1, 5, -1, 0, None, None, None, None, None, None) == 0


def test_python_argument_checks():
    m = sa.ScrappyMatrix.from_numpy(np.zeros((4, 25), dtype=np.float32), sloika=False)
    with pytest.raises(ValueError):
        sa.map_trans_to_reference(m, "ACGT", viterbi=False, path=True)
    with pytest.raises(TypeError):
        sa.map_trans_to_reference(np.zeros((4, 25), dtype=np.float32), "ACGT")
    with pytest.raises(ValueError):
        sa.map_trans_to_reference(sa.ScrappyMatrix.from_numpy(np.zeros((4, 5), dtype=np.float32), sloika=False), "ACGT")
    with pytest.raises(ValueError):
        sa.map_trans_to_reference(m, "ACN")

    class NoEngine(object):
        def __getattr__(self, name):
            raise AssertionError("the argument checks reached the engine (%s)" % name)
    sigs = [np.zeros(1000, dtype=np.float32)] * 3
    with pytest.raises(ValueError, match="viterbi"):
        sa.Engine.map_to_reference(NoEngine(), sigs, "ACGT", viterbi=False, path=True)
    with pytest.raises(ValueError, match="per signal"):
        sa.Engine.map_to_reference(NoEngine(), sigs, ["ACGT", "ACGT"])


def test_planner_under_sanitizers(tmp_path):
    """tests/map_crf_local_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the planner on arrays of
    exactly as many entries as it says it writes"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "map_crf_local_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "map_crf_local_asan.c"),
                        os.path.join(csrc, "sh_host.c"), "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]
