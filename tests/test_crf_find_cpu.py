"""Short sequences searched inside flip-flop reads (k_crf_find, csrc/sh_crf_find.h): the restatement np_crf_find of the definition in
float32 with its own traceback, the checker that walks the path it returns, the identities that hold the definition (a run of the
read's own call scores decode_crf's score in bits; call_score is decode_crf's; score <= call_score; score >= the global mapping's),
the hand-worked all-zero cases, the planner of the packs (also under sanitizers, from its own program) and the argument checks of
`find_in_trans`.  No device is needed here; tests/test_gpu_crf_find.py holds the kernel against this restatement."""
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from test_map_crf_cpu import call_of, map_crf_cases, np_decode_crf, np_map_crf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = np.float32(1e30)
NEW_SYMBOLS = ("scrappie_hip_find_batch", "scrappie_hip_free_find_results", "find_crf_sequences_viterbi", "scrappie_hip_crf_find_plan",
               "scrappie_hip_crf_find_max_cells", "scrappie_hip_crf_find_form_counts")


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def np_crf_find(trans, motif):
    """The definition: trans [nblock][25] (element to * 5 + from, states A C G T stay), motif: L >= 1 bases coded 0..3.  Lattice at
    an entry: U[s] (no motif base yet, decode_crf's row), B[p] / S[p] for p = 1 .. L - 1 (p motif bases emitted, the entry is base
    m[p - 1] / a stay), V[s] (all L emitted).  float32 as tr + prev, candidates in the order written, replaced on strict > (argmax
    returns the first maximum).  Returns dict(score, begin, end, call_score, path): path holds the states of all nblock + 1
    entries from this function's own traceback; score NaN (begin = end = -1, path None) below -1e30 / 2."""
    tr_all = np.ascontiguousarray(trans, dtype=np.float32)
    m = np.asarray(motif, dtype=np.int64)
    NB, L = tr_all.shape[0], len(m)
    assert tr_all.shape[1] == 25 and NB >= 1 and L >= 1 and m.min() >= 0 and m.max() <= 3
    nI = L - 1                                           # interior cells: index i is p = i + 1
    ar = np.arange(5)
    U = np.zeros(5, dtype=np.float32)
    B = np.full(nI, -BIG, dtype=np.float32)
    S = B.copy()
    bB = np.zeros(nI, dtype=np.int64)
    bS = bB.copy()
    V = np.full(5, -BIG, dtype=np.float32)
    Vb = np.zeros(5, dtype=np.int64)
    Ve = Vb.copy()
    if L >= 2:
        B[0] = 0
    else:
        V[m[0]] = 0
    tbU = np.zeros((NB, 5), dtype=np.int64)
    tbB = np.zeros((NB, nI), dtype=np.int64)             # cell 1: the U state it came from; beyond: 0 base, 1 stay predecessor
    tbS = np.zeros((NB, nI), dtype=np.int64)             # 0: from B[p], 1: from S[p]
    tbV = np.zeros((NB, 5), dtype=np.int64)              # 0..4: V[s]; 5: B[L - 1]; 6: S[L - 1]; 7 + s: U[s] (L == 1)
    last = int(m[L - 1])
    iB = 5 * m[1:L - 1] + m[0:L - 2] if nI >= 2 else None   # p = 2 .. L - 1: b = m[p - 1], the base before it m[p - 2]
    iBs = 5 * m[1:L - 1] + 4 if nI >= 2 else None
    iS = 20 + m[0:L - 1]
    with np.errstate(over="ignore"):
        for t in range(NB):
            tr = tr_all[t]
            M = tr.reshape(5, 5)                         # [to][from]
            sc = M + U[None, :]
            kU = np.argmax(sc, axis=1)
            nU = sc[ar, kU]
            tbU[t] = kU
            nB, nS, nbB, nbS = B.copy(), S.copy(), bB.copy(), bS.copy()
            if L >= 2:
                c = M[m[0]] + U
                k = int(np.argmax(c))
                nB[0], nbB[0], tbB[t, 0] = c[k], t + 1, k
                if nI >= 2:
                    x = tr[iB] + B[:-1]
                    y = tr[iBs] + S[:-1]
                    k = y > x
                    nB[1:] = np.where(k, y, x)
                    nbB[1:] = np.where(k, bS[:-1], bB[:-1])
                    tbB[t, 1:] = k
                x = tr[iS] + B
                y = tr[24] + S
                k = y > x
                nS = np.where(k, y, x)
                nbS = np.where(k, bS, bB)
                tbS[t] = k
            sc = M + V[None, :]
            kV = np.argmax(sc, axis=1)
            nV = sc[ar, kV]
            nVb, nVe = Vb[kV], Ve[kV]
            tbV[t] = kV
            if L >= 2:
                x = tr[5 * last + m[L - 2]] + B[-1]
                if x > nV[last]:
                    nV[last], nVb[last], nVe[last], tbV[t, last] = x, bB[-1], t + 1, 5
                y = tr[5 * last + 4] + S[-1]
                if y > nV[last]:
                    nV[last], nVb[last], nVe[last], tbV[t, last] = y, bS[-1], t + 1, 6
            else:
                for s in range(5):
                    c = tr[5 * last + s] + U[s]
                    if c > nV[last]:
                        nV[last], nVb[last], nVe[last], tbV[t, last] = c, t + 1, t + 1, 7 + s
            U, B, S, bB, bS, V, Vb, Ve = nU, nB, nS, nbB, nbS, nV, nVb, nVe
    call = np.float32(U[int(np.argmax(U))])
    s = int(np.argmax(V))
    score = np.float32(V[s])
    if score < -BIG / 2:
        return dict(score=np.float32("nan"), begin=-1, end=-1, call_score=call, path=None)
    path = np.zeros(NB + 1, dtype=np.int32)
    kind, at = "V", s                                    # at: the state (U, V) or the interior index (B, S)
    for t in range(NB, 0, -1):
        if kind == "V":
            path[t] = at
            code = int(tbV[t - 1, at])
            if code < 5:
                at = code
            elif code == 5:
                kind, at = "B", nI - 1
            elif code == 6:
                kind, at = "S", nI - 1
            else:
                kind, at = "U", code - 7
        elif kind == "B":
            path[t] = m[at]
            k = int(tbB[t - 1, at])
            if at == 0:
                kind, at = "U", k
            else:
                kind, at = ("S" if k else "B"), at - 1
        elif kind == "S":
            path[t] = 4
            if not tbS[t - 1, at]:
                kind = "B"
        else:
            path[t] = at
            at = int(tbU[t - 1, at])
    path[0] = at if kind in ("U", "V") else (m[at] if kind == "B" else 4)
    assert kind == "U" or (kind == "B" and at == 0) or (kind == "V" and L == 1 and at == m[0]), (kind, at)
    return dict(score=score, begin=int(Vb[s]), end=int(Ve[s]), call_score=call, path=path)


def check_find(trans, motif, res):
    """walk the path: its float32 chain is the score in bits, entries begin and end are bases, and the bases of [begin, end] spell
    the motif"""
    tr_all = np.ascontiguousarray(trans, dtype=np.float32)
    path, b, e = res["path"], res["begin"], res["end"]
    assert path is not None and len(path) == tr_all.shape[0] + 1
    acc = np.float32(0)
    for t in range(tr_all.shape[0]):
        acc = tr_all[t, 5 * path[t + 1] + path[t]] + acc
    assert np.float32(acc).tobytes() == np.float32(res["score"]).tobytes(), (acc, res["score"])
    assert 0 <= b <= e <= tr_all.shape[0] and path[b] != 4 and path[e] != 4, (b, e)
    inside = path[b:e + 1]
    assert np.array_equal(inside[inside != 4], np.asarray(motif)), (b, e)


def bits(x):
    return np.float32(x).tobytes()


def call_motifs(seq):
    """the motifs of a call that must score decode_crf's score: the whole call, its first and last min(L, 1 / 2 / 7) bases, a
    middle slice, every single base of it"""
    L = len(seq)
    out = [("whole", seq)]
    for k in (1, 2, 7):
        out.append(("first-%d" % k, seq[:min(L, k)]))
        out.append(("last-%d" % k, seq[L - min(L, k):]))
    out.append(("middle", seq[L // 3:L // 3 + max(1, min(L // 3, 25))]))
    for b in sorted(set(int(x) for x in seq)):
        out.append(("base-%d" % b, np.array([b])))
    return out


_cases = []


def cases():
    if not _cases:
        _cases.extend(map_crf_cases())
    return _cases


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    for name in NEW_SYMBOLS:
        assert hasattr(sa.lib(), name), name
    assert set(sa.crf_find_form_counts()) == {(p, t) for p in (False, True) for t in (False, True)}
    # two columns of transitions (64 floats); per cell and the spare slot two buffers of (value, stay, begin, end) and a word
    assert sa.crf_find_max_cells() == (65536 - 4 * 64) // 36 - 1


def test_runs_of_the_call_score_decode_crf():
    n = 0
    for c in cases():
        if not c["from_call"]:
            continue
        n += 1
        for name, mo in call_motifs(c["seq"]):
            r = np_crf_find(c["trans"], mo)
            assert bits(r["score"]) == bits(c["dscore"]), (c["name"], name, r["score"], c["dscore"])
            assert bits(r["call_score"]) == bits(c["dscore"]), (c["name"], name)
            check_find(c["trans"], mo, r)
    assert n == 24


def test_call_score_is_decode_crf_on_every_case():
    for c in cases():
        ds, _ = np_decode_crf(c["trans"])
        r = np_crf_find(c["trans"], c["seq"][:1])
        assert bits(r["call_score"]) == bits(ds), c["name"]


def test_random_motifs_lie_between_the_global_score_and_the_call():
    rng = np.random.default_rng(11)
    n_global = 0
    for c in cases():
        nb = c["trans"].shape[0]
        if nb > 200:
            continue
        for L in sorted(set(min(x, nb + 1) for x in (1, 2, 3, 12, nb + 1))):
            mo = rng.integers(0, 4, L)
            r = np_crf_find(c["trans"], mo)
            assert not np.isnan(r["score"]), (c["name"], L)
            assert r["score"] <= r["call_score"], (c["name"], L)
            check_find(c["trans"], mo, r)
            g, _ = np_map_crf(c["trans"], mo)
            if not np.isnan(g):
                n_global += 1
                assert r["score"] >= np.float32(g), (c["name"], L, r["score"], g)
    assert n_global > 50


def test_the_only_path_is_the_global_mapping():
    n = 0
    for c in cases():
        nb = c["trans"].shape[0]
        if len(c["seq"]) != nb + 1:
            continue
        n += 1
        r = np_crf_find(c["trans"], c["seq"])
        g, gp = np_map_crf(c["trans"], c["seq"])
        assert bits(r["score"]) == bits(g), c["name"]
        assert (r["begin"], r["end"]) == (0, nb)
        check_find(c["trans"], c["seq"], r)
    assert n >= 2                                        # only-path, only-path-1
    rng = np.random.default_rng(5)
    for nb in (1, 2, 3, 9):
        tr = rng.normal(0, 2, (nb, 25)).astype(np.float32)
        mo = rng.integers(0, 4, nb + 1)
        assert bits(np_crf_find(tr, mo)["score"]) == bits(np_map_crf(tr, mo)[0])


def test_a_motif_longer_than_the_entries_fits_nowhere():
    rng = np.random.default_rng(6)
    for nb in (1, 2, 3, 17):
        tr = rng.normal(0, 2, (nb, 25)).astype(np.float32)
        r = np_crf_find(tr, rng.integers(0, 4, nb + 2))
        assert np.isnan(r["score"]) and r["path"] is None and (r["begin"], r["end"]) == (-1, -1)
        assert bits(r["call_score"]) == bits(np_decode_crf(tr)[0])
    c = [x for x in cases() if x["name"] == "no-path"][0]
    assert np.isnan(np_crf_find(c["trans"], c["seq"])["score"])


def test_all_zero_matrix_by_hand():
    """NB = 3, every transition 0: every path scores 0 and the tie order decides.
    L = 1, motif [2]: entry 0 holds V[2] = 0 with (begin, end) = (0, 0).  Block 0: every V'[s'] takes the continuation, whose first
    candidate above -1e30 is V[2]: 0 with (0, 0); the emission from U into V'[2] offers 0, not > 0.  From then on all five V cells
    are 0 with (0, 0), continuations tie and keep the first, emissions never exceed.  End: V[0] first: score 0, begin 0, end 0.
    L = 2, motif [1, 3]: entry 0 holds B[1] = 0 (begin 0).  Block 0: continuations are -1e30; V'[3] takes the emission from B[1]:
    0 > -1e30 with begin 0, end 1 (B'[1] restarts at 0 with begin 1, S'[1] = 0 from B[1] with begin 0).  Block 1: every V'[s'] takes
    V[3]: 0 with (0, 1); the emissions into V'[3] offer 0, not > 0.  Block 2 likewise.  End: V[0]: score 0, begin 0, end 1."""
    z = np.zeros((3, 25), dtype=np.float32)
    r = np_crf_find(z, [2])
    assert (bits(r["score"]), r["begin"], r["end"]) == (bits(0.0), 0, 0) and bits(r["call_score"]) == bits(0.0)
    check_find(z, [2], r)
    r = np_crf_find(z, [1, 3])
    assert (bits(r["score"]), r["begin"], r["end"]) == (bits(0.0), 0, 1)
    check_find(z, [1, 3], r)
    for c in cases():
        if c["name"].startswith("all-zero"):
            r = np_crf_find(c["trans"], c["seq"])
            assert (bits(r["score"]), r["begin"]) == (bits(0.0), 0) and r["end"] == len(c["seq"]) - 1, c["name"]
            check_find(c["trans"], c["seq"], r)


def test_planner():
    maxc = sa.crf_find_max_cells()
    rng = np.random.default_rng(3)
    assert sa.crf_find_plan([], 256)[0] == 0                                     # sizes 0 and 1
    npk, pack, cell = sa.crf_find_plan([40], 256)
    assert (npk, list(pack), list(cell)) == (1, [0], [5])
    npk, pack, cell = sa.crf_find_plan([40] * 24, 256)                           # five motifs of 44 cells behind the read's five
    assert npk == 5 and list(pack) == [k // 5 for k in range(24)] and list(cell) == [5 + 44 * (k % 5) for k in range(24)]
    for pc in (0, 1, 14, 64, 128, 256, 257, 1024, maxc, maxc + 1, 1 << 40):
        ln = rng.integers(1, 90, 200)
        ln[rng.integers(0, 200, 6)] = maxc - 8                                   # over the maximum: L + 9 > maxc
        ln[rng.integers(0, 200, 3)] = maxc - 9                                   # the longest that fits, alone in its pack
        ln[rng.integers(0, 200, 3)] = 0
        npk, pack, cell = sa.crf_find_plan(ln, pc)
        lim = min(pc, maxc)
        over = (ln == 0) | (ln + 9 > maxc)
        assert np.all(pack[over] == -1) and np.all(cell[over] == -1) and np.all(pack[~over] >= 0)
        kept = np.flatnonzero(~over)
        assert np.all(np.diff(pack[kept]) >= 0) and np.all(np.diff(pack[kept]) <= 1) and npk == pack[kept].max() + 1      # input order
        for p in range(npk):
            mem = kept[pack[kept] == p]
            ends = 5 + np.cumsum(ln[mem] + 4)
            assert list(cell[mem]) == [5] + list(ends[:-1]), (pc, p)
            assert ends[-1] <= maxc and (ends[-1] <= lim or len(mem) == 1), (pc, p)
            if p + 1 < npk:                                                      # closed only because the next motif would pass pack_cells
                nxt = kept[pack[kept] == p + 1][0]
                assert ends[-1] + ln[nxt] + 4 > lim, (pc, p)


def test_planner_under_sanitizers(tmp_path):
    """tests/crf_find_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "crf_find_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "crf_find_asan.c"), os.path.join(csrc, "sh_host.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]


def test_find_in_trans_arguments():
    m = sa.ScrappyMatrix.from_numpy(np.zeros((4, 25), dtype=np.float32), sloika=False)
    with pytest.raises(TypeError):
        sa.find_in_trans(np.zeros((4, 25), dtype=np.float32), ["ACG"])
    with pytest.raises(ValueError):
        sa.find_in_trans(sa.ScrappyMatrix.from_numpy(np.zeros((4, 5), dtype=np.float32), sloika=False), ["ACG"])
    with pytest.raises(ValueError):
        sa.find_in_trans(m, ["ACG", ""])
    with pytest.raises(ValueError):
        sa.find_in_trans(m, ["ACN"])
