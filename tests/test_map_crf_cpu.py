"""Reads of a flip-flop (CRF) model mapped to base sequences (k_map_crf, sh_map_crf.h), the part that needs no GPU: the numpy
restatement of the recursion (np_map_crf: include/scrappie_hip.h states it), decode_crf restated (np_decode_crf) and, where it is
built, the compiled reference's; the cases both GPU pins are checked on; the host functions (band checker, diagonal band, scratch
plan, exports) and tests/map_crf_asan.c, a program of its own over sh_host.c under the address and undefined-behaviour sanitizers.

The pin needs no tolerance: mapping a read to the sequence decode_crf calls for it returns decode_crf's score in bits and its path
(float addition is monotone: the constrained optimum ranges over a subset of decode_crf's paths, and is at least the sequential sum
along decode_crf's own traceback path, which is decode_crf's score)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import scrappie_amd as sa
from test_map_cpu import check_scratch_plan, ref_decode_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1e30
NEW_SYMBOLS = ("map_crf_to_sequence_viterbi", "map_crf_to_sequence_forward", "map_crf_to_sequence_viterbi_banded",
               "map_crf_to_sequence_forward_banded", "scrappie_hip_map_crf_bounds_sane", "scrappie_hip_map_crf_diagonal_band",
               "scrappie_hip_map_crf_lds_max_seq", "scrappie_hip_map_crf_plan_scratch", "scrappie_hip_map_crf_form_counts")


# ---------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------
def _lse(x, y):
    """util.h:162-164 in the dtype of its arguments"""
    return np.maximum(x, y) + np.log1p(np.exp(-np.abs(x - y)))


def np_map_crf(trans, seq, viterbi=True, low=None, high=None, dtype=np.float32):
    """The specification: trans [nblock][25] (element to * 5 + from, states A C G T stay), seq: L bases coded 0..3.  Cells after
    entry t: B[p] (entry t was base seq[p - 1]) and S[p] (a stay), p = bases emitted so far.  Entry 0: B[1] = S[0] = 0.  Block t:
        B'[p] = max(tr[5 b + seq[p - 2]] + B[p - 1]  (p >= 2),  tr[5 b + 4] + S[p - 1]),   b = seq[p - 1]
        S'[p] = max(tr[20 + b] + B[p]                (p >= 1),  tr[24] + S[p])
    the base predecessor first, stay on strict >; forward: _lse in the same order.  Band: cell p of entry t in [low[t], high[t])
    (nblock + 1 entries each), everything outside a complete row's band is -1e30; None: the full band.  Vectorised over the cells
    of an entry's band.  Returns (score, path): path[t] = last base emitted through entry t (-1: none), None for forward; a score
    below -1e30 / 2 is (nan, None)."""
    tr_all = np.ascontiguousarray(trans, dtype=dtype)
    seq = np.asarray(seq, dtype=np.int64)
    NB, L = tr_all.shape[0], len(seq)
    assert tr_all.shape[1] == 25 and NB >= 1 and L >= 1
    big = dtype(BIG)
    b = np.zeros(L + 1, dtype=np.int64)
    b[1:] = seq
    bp = np.zeros(L + 1, dtype=np.int64)
    bp[2:] = seq[:-1]
    iBB, iBS, iSB = 5 * b + bp, 5 * b + 4, 20 + b
    B = np.full(L + 1, -big, dtype=dtype)
    S = B.copy()
    S[0] = 0
    if low is None or int(high[0]) > 1:
        B[1] = 0
    if viterbi:
        KB = np.zeros((NB, L + 1), dtype=bool)
        KS = np.zeros((NB, L + 1), dtype=bool)
    with np.errstate(over="ignore"):
        for t in range(NB):
            lo, hi = (0, L + 1) if low is None else (int(low[t + 1]), int(high[t + 1]))
            tr = tr_all[t]
            nB = np.full(L + 1, -big, dtype=dtype)
            nS = nB.copy()
            a = max(lo, 1)
            if a < hi:
                base = tr[iBB[a:hi]] + B[a - 1:hi - 1]
                stay = tr[iBS[a:hi]] + S[a - 1:hi - 1]
                if viterbi:
                    k = stay > base
                    if a == 1:
                        k[0] = True                     # B'[1] has the stay predecessor only
                    nB[a:hi] = np.where(k, stay, base)
                    KB[t, a:hi] = k
                else:
                    v = _lse(base, stay)
                    if a == 1:
                        v[0] = stay[0]
                    nB[a:hi] = v
            sb = tr[iSB[lo:hi]] + B[lo:hi]
            ss = tr[24] + S[lo:hi]
            if viterbi:
                k = ss > sb
                if lo == 0:
                    k[0] = True                         # S'[0] likewise
                nS[lo:hi] = np.where(k, ss, sb)
                KS[t, lo:hi] = k
            else:
                v = _lse(sb, ss)
                if lo == 0:
                    v[0] = ss[0]
                nS[lo:hi] = v
            B, S = nB, nS
        xb, xs = B[L], S[L]
        score = (xb if xb >= xs else xs) if viterbi else _lse(xb, xs)
    if score < -big / 2:
        return float("nan"), None
    if not viterbi:
        return score, None
    path = np.zeros(NB + 1, dtype=np.int32)
    p, kind = L, (0 if xb >= xs else 1)
    for t in range(NB, 0, -1):
        path[t] = p - 1
        stay = (KS if kind else KB)[t - 1, p]
        if kind == 0:
            p -= 1
        kind = 1 if stay else 0
    path[0] = p - 1
    return score, path


def np_decode_crf(trans):
    """decode.c:836-893 in float32: (score, path of nblock + 1 states)"""
    tr_all = np.ascontiguousarray(trans, dtype=np.float32)
    NB = tr_all.shape[0]
    prev = np.zeros(5, dtype=np.float32)
    tb = np.zeros((NB, 5), dtype=np.int32)
    for t in range(NB):
        sc = tr_all[t].reshape(5, 5) + prev[None, :]    # [to][from]
        tb[t] = np.argmax(sc, axis=1)                   # the first maximum: from-state ascending, replaced on strict >
        prev = sc[np.arange(5), tb[t]]
    path = np.zeros(NB + 1, dtype=np.int32)
    path[NB] = int(np.argmax(prev))
    for t in range(NB, 0, -1):
        path[t - 1] = tb[t - 1, path[t]]
    return np.float32(prev[path[NB]]), path


def ref_decode_crf(trans):
    """the compiled reference's decode_crf (oracle/_ref/libref_decode.so); None where it is not built"""
    R = ref_decode_lib()
    if R is None:
        return None
    R.decode_crf.restype = C.c_float
    R.decode_crf.argtypes = [C.POINTER(oracle.Mat), C.POINTER(C.c_int)]
    m = oracle.NpMat(np.ascontiguousarray(trans, dtype=np.float32))
    path = np.zeros(trans.shape[0] + 1, dtype=np.int32)
    s = R.decode_crf(m.ptr, path.ctypes.data_as(C.POINTER(C.c_int)))
    return np.float32(s), path


def call_of(dpath):
    """(seq, path) of a decode_crf path: its non-stay entries, and per entry the index of the last base emitted"""
    base = np.asarray(dpath) != 4
    return np.asarray(dpath)[base].astype(np.int32), (np.cumsum(base) - 1).astype(np.int32)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def _trans(nblock, sigma, rng):
    t = rng.normal(0.0, sigma, (nblock, 25)).astype(np.float32)
    t[:, 24] += np.float32(1.5)                     # stay -> stay: calls shorter than the reads
    return t


def _case(name, trans, seq, from_call=False, dscore=None, dpath=None):
    return dict(name=name, trans=trans, seq=np.asarray(seq, dtype=np.int32), from_call=from_call, dscore=dscore, dpath=dpath)


def map_crf_cases():
    """fixed seeds.  from_call: the sequence is decode_crf's own call of the matrix (dscore, dpath: its score and the path that
    mapping must return)."""
    out = []
    for si, sigma in enumerate((0.5, 2.0, 6.0)):
        for nblock in (1, 2, 3, 5, 17, 64, 200, 800):
            seed = 1000 * (si + 1) + nblock
            while True:                             # a call of no base at all (short reads) is no sequence: the next seed
                trans = _trans(nblock, sigma, np.random.default_rng(seed))
                ds, dp = np_decode_crf(trans)
                seq, path = call_of(dp)
                if len(seq) >= 1:
                    break
                seed += 100000
            out.append(_case("call-s%g-n%d" % (sigma, nblock), trans, seq, True, ds, path))
    rng = np.random.default_rng(7)
    out.append(_case("one-base-800", _trans(800, 2.0, rng), [2]))
    out.append(_case("only-path", _trans(17, 2.0, rng), rng.integers(0, 4, 18)))
    out.append(_case("only-path-1", _trans(1, 2.0, rng), [3, 0]))
    out.append(_case("no-path", _trans(17, 2.0, rng), rng.integers(0, 4, 19)))
    out.append(_case("homopolymer-A", _trans(64, 2.0, rng), [0] * 10))
    out.append(_case("homopolymer-T", _trans(40, 0.5, rng), [3] * 33))
    for cells in (63, 64, 65, 255, 256, 257, 513):  # a wave and a chunk of threads from both sides
        L = cells - 1
        out.append(_case("cells-%d" % cells, _trans(L + 1 + cells % 7 if cells < 200 else 2 * L, 2.0, rng), rng.integers(0, 4, L)))
    out.append(_case("all-zero", np.zeros((20, 25), dtype=np.float32), rng.integers(0, 4, 7)))
    out.append(_case("all-zero-homopolymer", np.zeros((9, 25), dtype=np.float32), [1] * 5))
    return out


def crf_lds_max_seq():
    return int(sa.lib().scrappie_hip_map_crf_lds_max_seq())


def map_crf_scratch_cases():
    """sequences around the LDS home's last length M: M itself (LDS), M + 1, M + 2, M + 600 (scratch), each against a read of just
    more blocks than bases and against one of twice as many"""
    M = crf_lds_max_seq()
    rng = np.random.default_rng(11)
    out = []
    for L in (M, M + 1, M + 2, M + 600):
        for nblock in (L + 2, 2 * L):
            out.append(_case("scratch-L%d-n%d" % (L, nblock), _trans(nblock, 2.0, rng), rng.integers(0, 4, L)))
    return out


def path_bands(path, L, which):
    """bands from a Viterbi path (cells cnt[t] = path[t] + 1), all valid: 'around' [cnt - 1, cnt + 2); 'low-edge' the low edge
    is the path, 5 cells wide; 'high-edge' the high edge is the path; 'exact' the path alone (width 1 behind entry 0);
    'stall-slide' the low edge stalls, then slides by 3, 8 cells wide"""
    cnt = np.asarray(path, dtype=np.int64) + 1
    if which == "around":
        lo, hi = cnt - 1, cnt + 2
    elif which == "low-edge":
        lo, hi = cnt.copy(), cnt + 5
    elif which == "high-edge":
        lo, hi = cnt - 4, cnt + 1
    elif which == "exact":
        lo, hi = cnt.copy(), cnt + 1
    elif which == "stall-slide":
        lo = (np.maximum(cnt - 3, 0) // 3) * 3
        hi = lo + 8
    else:
        raise ValueError(which)
    lo = np.clip(lo, 0, L)
    lo[0] = 0
    hi = np.clip(hi, 1, L + 1)
    return lo.astype(np.uintp), hi.astype(np.uintp)


def no_path_band(nblock, L):
    """valid, and nothing gets through: three cells wide, sliding by three at every entry"""
    lo = np.minimum(3 * np.arange(nblock + 1), L - 2)
    return lo.astype(np.uintp), (lo + 3).astype(np.uintp)


def bounds_sane(lo, hi, nblock, L):
    sp = C.POINTER(C.c_size_t)
    lo, hi = (np.ascontiguousarray(x, dtype=np.uintp) for x in (lo, hi))
    return bool(sa.lib().scrappie_hip_map_crf_bounds_sane(lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), nblock, L))


def np_bounds_sane(lo, hi, nblock, L):
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    if len(lo) != nblock + 1 or len(hi) != nblock + 1 or lo[0] != 0 or hi[nblock] != L + 1:
        return False
    if np.any(lo >= hi) or np.any(hi > L + 1):
        return False
    return bool(np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0) and np.all(lo[1:] <= hi[:-1]))


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    for name in NEW_SYMBOLS:
        assert hasattr(sa.lib(), name), name
    assert set(sa.map_crf_form_counts()) == {(v, t, s) for v in (False, True) for t in (False, True) for s in (False, True)}
    assert crf_lds_max_seq() == (65536 - 4 * (64 + 8)) // 20          # 64 floats of transitions, 4 (L + 2) of rows, L codes


def test_np_decode_crf_is_the_reference():
    if ref_decode_lib() is None:
        pytest.skip("oracle/_ref/libref_decode.so is not built")
    for c in map_crf_cases():
        ws, wp = ref_decode_crf(c["trans"])
        gs, gp = np_decode_crf(c["trans"])
        assert np.float32(gs).tobytes() == ws.tobytes() and np.array_equal(gp, wp), c["name"]


def test_mapping_a_call_is_decode_crf():
    """a condition on the fixtures: for every case made from a call the restatement returns decode_crf's score in bits and its
    path, unbanded, in the band [cnt - 1, cnt + 2) around the path and in every other band made from the path"""
    n = 0
    for c in map_crf_cases():
        if not c["from_call"]:
            continue
        n += 1
        L, nb = len(c["seq"]), c["trans"].shape[0]
        s, p = np_map_crf(c["trans"], c["seq"])
        assert np.float32(s).tobytes() == np.float32(c["dscore"]).tobytes(), (c["name"], s, c["dscore"])
        assert np.array_equal(p, c["dpath"]), c["name"]
        for which in ("around", "low-edge", "high-edge", "exact", "stall-slide"):
            lo, hi = path_bands(p, L, which)
            assert np_bounds_sane(lo, hi, nb, L) and bounds_sane(lo, hi, nb, L), (c["name"], which)
            s2, p2 = np_map_crf(c["trans"], c["seq"], low=lo, high=hi)
            assert np.float32(s2).tobytes() == np.float32(s).tobytes() and np.array_equal(p2, p), (c["name"], which)
    assert n == 24


def test_restatement_on_the_hand_made_cases():
    cases = {c["name"]: c for c in map_crf_cases()}
    s, p = np_map_crf(cases["no-path"]["trans"], cases["no-path"]["seq"])
    assert np.isnan(s) and p is None
    for name in ("only-path", "only-path-1"):           # every entry a base: the sum of its transitions, in order
        c = cases[name]
        s, p = np_map_crf(c["trans"], c["seq"])
        want = np.float32(0)
        for t in range(c["trans"].shape[0]):
            want = np.float32(c["trans"][t, 5 * c["seq"][t + 1] + c["seq"][t]] + want)
        assert np.float32(s).tobytes() == want.tobytes() and np.array_equal(p, np.arange(len(c["seq"])))
        lo = np.arange(len(c["seq"]), dtype=np.uintp) + 1
        lo[0] = 0
        hi = np.arange(len(c["seq"]), dtype=np.uintp) + 2       # width 1 behind entry 0: the one path there is
        assert bounds_sane(lo, hi, c["trans"].shape[0], len(c["seq"]))
        s2, p2 = np_map_crf(c["trans"], c["seq"], low=lo, high=hi)
        assert np.float32(s2).tobytes() == want.tobytes() and np.array_equal(p2, p)
    c = cases["one-base-800"]
    s, p = np_map_crf(c["trans"], c["seq"])
    assert np.isfinite(s) and set(p.tolist()) <= {-1, 0} and p[-1] == 0 and np.all(np.diff(p) >= 0)
    # all-zero: every path ties at 0; a base is taken as early as the order of the candidates allows (the base predecessor
    # first, stay only on strict >; a base at the end on a tie): the walk back from B[L] takes bases all the way down
    c = cases["all-zero"]
    s, p = np_map_crf(c["trans"], c["seq"])
    nb, L = 20, 7
    assert s == 0 and p.tolist() == [-1] * (nb + 1 - L) + list(range(L))
    f32, _ = np_map_crf(c["trans"], c["seq"], viterbi=False)
    f64, _ = np_map_crf(c["trans"], c["seq"], viterbi=False, dtype=np.float64)
    import math
    assert abs(float(f64) - math.log(math.comb(nb + 1, L))) < 1e-9          # the paths: which L of the nb + 1 entries are bases
    assert abs(float(f32) - float(f64)) < 1e-4
    for c in map_crf_cases():                              # a band that lets nothing through
        L, nb = len(c["seq"]), c["trans"].shape[0]
        if L < 9 or nb < 4 or 3 * nb < L - 2:
            continue
        lo, hi = no_path_band(nb, L)
        assert bounds_sane(lo, hi, nb, L), c["name"]
        assert np.isnan(np_map_crf(c["trans"], c["seq"], low=lo, high=hi)[0]), c["name"]
        assert np.isnan(np_map_crf(c["trans"], c["seq"], viterbi=False, low=lo, high=hi)[0]), c["name"]


def test_the_full_band_is_no_band():
    for c in map_crf_cases():
        L, nb = len(c["seq"]), c["trans"].shape[0]
        if nb > 200:
            continue
        lo, hi = np.zeros(nb + 1, dtype=np.uintp), np.full(nb + 1, L + 1, dtype=np.uintp)
        for vit in (True, False):
            a, b = np_map_crf(c["trans"], c["seq"], viterbi=vit), np_map_crf(c["trans"], c["seq"], viterbi=vit, low=lo, high=hi)
            assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes(), c["name"]
            assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1]), c["name"]


def test_scratch_cases_straddle_the_threshold():
    M = crf_lds_max_seq()
    cases = map_crf_scratch_cases()
    assert sorted({len(c["seq"]) for c in cases}) == [M, M + 1, M + 2, M + 600]
    assert all(c["trans"].shape[0] in (len(c["seq"]) + 2, 2 * len(c["seq"])) for c in cases) and len(cases) == 8
    off, _ = sa.plan_scratch("map_crf", [len(c["seq"]) for c in cases], [c["trans"].shape[0] for c in cases])
    assert [int(o) >= 0 for o in off] == [len(c["seq"]) > M for c in cases]


def test_bounds_checker():
    nb, L = 6, 4
    lo = np.array([0, 0, 1, 1, 2, 3, 3], dtype=np.uintp)
    hi = np.array([2, 2, 3, 4, 5, 5, 5], dtype=np.uintp)
    assert bounds_sane(lo, hi, nb, L) and np_bounds_sane(lo, hi, nb, L)
    assert bounds_sane(np.zeros(nb + 1), np.full(nb + 1, L + 1), nb, L)
    sp = C.POINTER(C.c_size_t)
    assert not sa.lib().scrappie_hip_map_crf_bounds_sane(None, hi.ctypes.data_as(sp), nb, L)
    assert not sa.lib().scrappie_hip_map_crf_bounds_sane(lo.ctypes.data_as(sp), None, nb, L)
    assert not sa.lib().scrappie_hip_map_crf_bounds_sane(lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), 0, L)
    assert not sa.lib().scrappie_hip_map_crf_bounds_sane(lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), nb, 0)

    def bad(i, l=None, h=None):
        a, b = lo.copy(), hi.copy()
        if l is not None:
            a[i] = l
        if h is not None:
            b[i] = h
        assert not np_bounds_sane(a, b, nb, L), (i, l, h)
        assert not bounds_sane(a, b, nb, L), (i, l, h)
    bad(0, l=1)                 # does not start at cell 0
    bad(nb, h=4)                # does not end with cell L
    bad(nb, h=6)                # beyond L + 1
    bad(3, h=6)
    bad(2, l=3)                 # empty
    bad(2, l=4)                 # the wrong way round
    bad(3, l=0)                 # low decreases
    bad(3, h=2)                 # high decreases (and empty)
    bad(4, h=3)                 # high decreases
    a = np.array([0, 0, 3, 3, 3, 3, 3], dtype=np.uintp)        # low[2] > high[1]: no predecessor
    b = np.array([2, 2, 5, 5, 5, 5, 5], dtype=np.uintp)
    assert not np_bounds_sane(a, b, nb, L) and not bounds_sane(a, b, nb, L)
    rng = np.random.default_rng(3)
    for _ in range(300):         # the two statements agree on random near-bands
        nb, L = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        a = np.sort(rng.integers(0, L + 1, nb + 1))
        b = np.sort(rng.integers(1, L + 3, nb + 1))
        if rng.random() < 0.7:
            a[0], b[nb] = 0, L + 1
        assert bounds_sane(a, b, nb, L) == np_bounds_sane(a, b, nb, L), (a, b, nb, L)


def test_diagonal_band_is_always_valid():
    for nb in (1, 2, 3, 7, 40, 173):
        for L in range(1, nb + 2):
            for h in (0, 1, 2, 5, 1000):
                lo, hi = sa.map_crf_diagonal_band(nb, L, h)
                assert len(lo) == nb + 1 and np_bounds_sane(lo, hi, nb, L) and bounds_sane(lo, hi, nb, L), (nb, L, h)
                d = (np.arange(nb + 1) * L) // nb
                assert np.all(lo <= d) and np.all(d < hi), (nb, L, h)       # the diagonal is inside
                assert np.all(hi.astype(np.int64) - lo.astype(np.int64) <= 2 * h + 2), (nb, L, h)
    lo, hi = sa.map_crf_diagonal_band(5, 40, 0)            # steeper than any path: still a valid band
    assert np_bounds_sane(lo, hi, 5, 40)
    with pytest.raises(ValueError):
        sa.map_crf_diagonal_band(0, 4, 1)


def test_scratch_plan_keeps_neighbours_apart():
    """map_crf_plan_add: k_map_crf touches 4 (L + 2) floats from a read's scratch offset (two buffers of a B row and an S row,
    cells 0 .. L and the spare slot)"""
    M = crf_lds_max_seq()
    lens = [M + 1, M + 2, 7, M + 3, M + 4, M, M + 1, M + 600, M - 1, M + 5, 65536]
    rng = np.random.default_rng(23)
    for order in (np.arange(len(lens)), np.arange(len(lens))[::-1], rng.permutation(len(lens))):
        L = [lens[i] for i in order]
        check_scratch_plan("map_crf", L, [1 + (i % 41) for i in range(len(L))], lambda n: n <= M, lambda n: 4 * (n + 2))
    for L in (M + 1, M + 2):                                # a lone read: the allocation covers it
        check_scratch_plan("map_crf", [L], [40], lambda n: n <= M, lambda n: 4 * (n + 2))


def test_map_trans_to_sequence_arguments():
    m = sa.ScrappyMatrix.from_numpy(np.zeros((4, 25), dtype=np.float32), sloika=False)
    with pytest.raises(ValueError):
        sa.map_trans_to_sequence(m, "ACG", viterbi=False, path=True)
    with pytest.raises(TypeError):
        sa.map_trans_to_sequence(np.zeros((4, 25), dtype=np.float32), "ACG")
    with pytest.raises(ValueError):
        sa.map_trans_to_sequence(sa.ScrappyMatrix.from_numpy(np.zeros((4, 5), dtype=np.float32), sloika=False), "ACG")
    with pytest.raises(ValueError):
        sa.map_trans_to_sequence(m, "ACN")
    with pytest.raises(ValueError):
        sa.map_trans_to_sequence(m, "ACG", bands=(np.zeros(4), np.full(4, 4)))          # one entry per block only
    with pytest.raises(ValueError):
        sa.map_trans_to_sequence(m, "ACG", bands=(np.ones(5), np.full(5, 4)))           # does not start at cell 0


def test_host_functions_under_sanitizers(tmp_path):
    """tests/map_crf_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the band checker and the diagonal
    band on arrays of exactly nblock + 1 entries"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "map_crf_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "map_crf_asan.c"), os.path.join(csrc, "sh_host.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]
