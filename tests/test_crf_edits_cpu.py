"""Every single-base edit of a sequence scored against a read of a flip-flop (CRF) model (k_crf_edits_rows, k_crf_edits,
csrc/sh_crf_edits.h), the part that needs no GPU.  np_crf_edits is the definition (include/scrappie_hip.h states it in words): the
forward rows of np_map_crf kept for every entry, backward rows, and per edit the join in the cell of the suffix's first base.  It
is held here against np_map_crf on the edited sequence (sa.apply_edit) -- in float64 to 1e-9, where the only difference is the
order of additions; in float32 within the project's standing bound for re-associated sums -- on calls, an only path, L = NB, a
homopolymer, one base and an all-zero matrix.  Further: the layout of a launch on the host (scrappie_hip_crf_edits_plan; under
sanitizers through tests/crf_edits_asan.c), the Python argument checks and the exports."""
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from test_map_crf_cpu import BIG, _lse, _trans, call_of, np_decode_crf, np_map_crf
from test_map_multi_cpu import _NoEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scrappie_hip_map_crf_edits_batch", "scrappie_hip_free_edits_results", "map_crf_edits", "scrappie_hip_crf_edits_pitch",
               "scrappie_hip_crf_edits_row_bytes", "scrappie_hip_crf_edits_plan", "scrappie_hip_crf_edits_form_counts",
               "scrappie_hip_crf_edits_timing")


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def np_crf_edits(trans, seq, viterbi=True, dtype=np.float32):
    """(base, sub (L, 4), dele (L,), ins (L + 1, 4)) in `dtype`; NaN where the edited sequence has no admissible path.
    mx(a, b): b if b > a else a (Viterbi), _lse(a, b) (forward), the arguments in the order of the definition.  The rows are
    vectorised over the cells of an entry, the edits over the positions i = 0 .. L."""
    tr_all = np.ascontiguousarray(trans, dtype=dtype)
    seq = np.asarray(seq, dtype=np.int64)
    NB, L = tr_all.shape[0], len(seq)
    assert tr_all.shape[1] == 25 and NB >= 1 and L >= 1
    big = dtype(BIG)

    def mx(a, b):
        return np.where(b > a, b, a) if viterbi else _lse(a, b)

    def end(x, y):
        return np.where(x >= y, x, y) if viterbi else _lse(x, y)

    with np.errstate(over="ignore", invalid="ignore"):
        # forward rows: cells 0 .. L (F_B[.][0] stays -BIG: there is no B[0])
        FB = np.full((NB + 1, L + 1), -big, dtype=dtype)
        FS = FB.copy()
        FB[0, 1] = 0
        FS[0, 0] = 0
        b = np.zeros(L + 1, dtype=np.int64)
        b[1:] = seq
        bp = np.zeros(L + 1, dtype=np.int64)
        bp[2:] = seq[:-1]
        for t in range(NB):
            tr = tr_all[t]
            stay = tr[5 * b[1:] + 4] + FS[t, :-1]
            move = tr[5 * b[1:] + bp[1:]] + FB[t, :-1]
            v = mx(move, stay)
            v[0] = stay[0]                                  # p == 1: the stay term alone
            FB[t + 1, 1:] = v
            v = mx(tr[20 + b] + FB[t], tr[24] + FS[t])
            v[0] = tr[24] + FS[t, 0]                        # p == 0 likewise
            FS[t + 1] = v
        base = end(FB[NB, L], FS[NB, L])
        # backward rows: cells 0 .. L + 1, column L + 1 is -BIG throughout
        GB = np.full((NB + 1, L + 2), -big, dtype=dtype)
        GS = GB.copy()
        GB[NB, L] = 0
        GS[NB, L] = 0
        nx = np.zeros(L + 1, dtype=np.int64)
        nx[:L] = seq                                        # seq[p], p < L
        for t in range(NB - 1, -1, -1):
            tr = tr_all[t]
            stB = tr[20 + b] + GS[t + 1, :L + 1]
            v = mx(tr[5 * nx + b] + GB[t + 1, 1:], stB)
            v[L] = stB[L]                                   # p == L: the second term alone
            v[0] = -big                                     # G_B needs 1 <= p
            GB[t, :L + 1] = v
            stS = tr[24] + GS[t + 1, :L + 1]
            v = mx(tr[5 * nx + 4] + GB[t + 1, 1:], stS)
            v[L] = stS[L]
            GS[t, :L + 1] = v
        # the edits, position i = 0 .. L at once
        i = np.arange(L + 1)
        hp = i >= 1
        pb = np.where(hp, seq[np.maximum(i - 1, 0)], 0)
        n0 = seq[np.minimum(i, L - 1)]                      # the suffix's first base of an insertion before i (i < L)
        n1 = seq[np.minimum(i + 1, L - 1)]                  # ... of a substitution or deletion at i (i < L - 1)
        G1 = GB[:, np.minimum(i + 1, L + 1)]                # G_B[t][i + 1]
        G2 = GB[:, np.minimum(i + 2, L + 1)]                # G_B[t][i + 2]
        XB = np.where(i == 0, dtype(0), -big)[None, :].repeat(4, axis=0).astype(dtype)
        XS = np.full((4, L + 1), -big, dtype=dtype)
        sub = (-big + G2[0])[None, :].repeat(4, axis=0)     # Y[0] = -BIG: the new base precedes n
        ins = (-big + G1[0])[None, :].repeat(4, axis=0)
        dele = np.where(i == 0, dtype(0), -big).astype(dtype) + G2[0]
        for t in range(NB):
            tr = tr_all[t]
            fb, fs = FB[t], FS[t]
            dS = tr[5 * n1 + 4] + fs
            yd = np.where(hp, mx(tr[5 * n1 + pb] + fb, dS), dS)
            dele = mx(dele, yd + G2[t + 1])
            for c in range(4):
                ys = mx(tr[5 * n1 + c] + XB[c], tr[5 * n1 + 4] + XS[c])
                sub[c] = mx(sub[c], ys + G2[t + 1])
                yi = mx(tr[5 * n0 + c] + XB[c], tr[5 * n0 + 4] + XS[c])
                ins[c] = mx(ins[c], yi + G1[t + 1])
                xS = tr[5 * c + 4] + fs
                nb = np.where(hp, mx(tr[5 * c + pb] + fb, xS), xS)
                ns = mx(tr[20 + c] + XB[c], tr[24] + XS[c])
                XB[c], XS[c] = nb, ns
        # no suffix: the end rule on the source's last cells
        closed = end(XB, XS)
        ins[:, L] = closed[:, L]
        sub[:, L - 1] = closed[:, L - 1]
        dele[L - 1] = end(FB[NB, L - 1], FS[NB, L - 1])
        if L == 1:
            dele[0] = np.nan                                # the empty sequence is none
        out = [np.asarray(base, dtype=dtype).reshape(1), sub[:, :L].T.copy(), dele[:L].copy(), ins.T.copy()]
        for a in out:
            a[a < -big / 2] = np.nan
    return dtype(out[0][0]), out[1], out[2], out[3]


def all_edits(seq):
    """(kind, i, c) of every single-base edit, and the result array it indexes"""
    L = len(seq)
    return ([("sub", i, c) for i in range(L) for c in range(4)] + [("del", i, None) for i in range(L)] +
            [("ins", i, c) for i in range(L + 1) for c in range(4)])


def pick(res, kind, i, c):
    base, sub, dele, ins = res
    return sub[i][c] if kind == "sub" else dele[i] if kind == "del" else ins[i][c]


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def crf_edits_cases():
    """(name, trans, seq), fixed seeds"""
    out = []
    for si, sigma in enumerate((0.5, 2.0, 6.0)):
        for nblock in (1, 2, 3, 5, 17, 40):
            seed = 5000 * (si + 1) + nblock
            while True:                                     # a call of no base at all is no sequence: the next seed
                trans = _trans(nblock, sigma, np.random.default_rng(seed))
                seq = call_of(np_decode_crf(trans)[1])[0]
                if len(seq) >= 1:
                    break
                seed += 100000
            out.append(("call-s%g-n%d" % (sigma, nblock), trans, seq))
    rng = np.random.default_rng(17)
    out.append(("only-path", _trans(17, 2.0, rng), rng.integers(0, 4, 18)))
    out.append(("L-equals-NB", _trans(12, 2.0, rng), rng.integers(0, 4, 12)))
    out.append(("homopolymer", _trans(30, 2.0, rng), [2] * 9))
    out.append(("one-base", _trans(9, 2.0, rng), [1]))
    out.append(("one-base-one-block", _trans(1, 2.0, rng), [3]))
    out.append(("all-zero", np.zeros((11, 25), dtype=np.float32), rng.integers(0, 4, 6)))
    return [(n, t, np.asarray(s, dtype=np.int32)) for n, t, s in out]


CASES = crf_edits_cases()


@pytest.fixture(scope="module")
def brute():
    """per case and form: the float64 and float32 scores of np_map_crf on every edited sequence, computed once"""
    out = {}
    for name, trans, seq in CASES:
        for vit in (True, False):
            f64, f32 = [], []
            for kind, i, c in all_edits(seq):
                ed = sa.apply_edit(seq, kind, i, c)
                if len(ed) == 0:
                    f64.append(np.nan), f32.append(np.nan)
                    continue
                f64.append(np_map_crf(trans, ed, viterbi=vit, dtype=np.float64)[0])
                f32.append(np_map_crf(trans, ed, viterbi=vit, dtype=np.float32)[0])
            out[name, vit] = (np.array(f64, dtype=np.float64), np.array(f32, dtype=np.float64))
    return out


# ---------------------------------------------------------------------------
# the definition against np_map_crf
# ---------------------------------------------------------------------------
def test_apply_edit():
    assert sa.apply_edit("ACGT", "sub", 1, "T") == "ATGT" and sa.apply_edit("ACGT", "sub", 3, 0) == "ACGA"
    assert sa.apply_edit("ACGT", "del", 0) == "CGT" and sa.apply_edit("ACGT", "del", 3) == "ACG"
    assert sa.apply_edit("ACGT", "ins", 0, "G") == "GACGT" and sa.apply_edit("ACGT", "ins", 4, 1) == "ACGTC"
    a = sa.apply_edit(np.array([0, 1, 2, 3]), "ins", 2, "T")
    assert a.dtype == np.int32 and a.tolist() == [0, 1, 3, 2, 3]
    assert sa.apply_edit([0, 1, 2, 3], "sub", 0, 2).tolist() == [2, 1, 2, 3] and sa.apply_edit([2], "del", 0).tolist() == []
    for bad in (("ACGT", "sub", 4, 0), ("ACGT", "del", 4, None), ("ACGT", "ins", 5, 0), ("ACGT", "sub", -1, 0), ("ACGT", "sub", 0, 4),
                ("ACGT", "sub", 0, "N"), ("ACGT", "ins", 0, None), ("ACGT", "swap", 0, 0)):
        with pytest.raises(ValueError):
            sa.apply_edit(*bad)


@pytest.mark.parametrize("viterbi", [True, False])
def test_float64_definition_equals_np_map_crf_of_every_edit(brute, viterbi):
    worst = 0.0
    for name, trans, seq in CASES:
        res = np_crf_edits(trans, seq, viterbi=viterbi, dtype=np.float64)
        want = brute[name, viterbi][0]
        got = np.array([pick(res, *e) for e in all_edits(seq)], dtype=np.float64)
        assert got.shape == want.shape == (9 * len(seq) + 4,)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, np.flatnonzero(np.isnan(got) != np.isnan(want)))
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
        if err.size:
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-9, (name, float(err.max()))
        w = np_map_crf(trans, seq, viterbi=viterbi, dtype=np.float64)[0]
        assert (np.isnan(w) and np.isnan(res[0])) or np.float64(res[0]).tobytes() == np.float64(w).tobytes(), name
    print("float64, %s: worst relative difference to np_map_crf of the edited sequence %.3g" % ("viterbi" if viterbi else "forward", worst))


@pytest.mark.parametrize("viterbi", [True, False])
def test_float32_definition_within_the_standing_bound(brute, viterbi):
    """|edits32 - f64| <= 2 |np_map_crf32(edited) - f64| + 1e-5 |f64|, base in bits"""
    worst, where = 0.0, None
    for name, trans, seq in CASES:
        res = np_crf_edits(trans, seq, viterbi=viterbi, dtype=np.float32)
        assert all(a.dtype == np.float32 for a in res[1:])
        f64, f32 = brute[name, viterbi]
        got = np.array([pick(res, *e) for e in all_edits(seq)], dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(f64)), name
        ok = ~np.isnan(f64)
        lhs = np.abs(got[ok] - f64[ok])
        rhs = 2 * np.abs(f32[ok] - f64[ok]) + 1e-5 * np.abs(f64[ok])
        assert np.all(lhs <= rhs), (name, float(np.max(lhs - rhs)))
        ratio = lhs / np.where(rhs > 0, rhs, 1.0)
        if ratio.size and ratio.max() > worst:
            worst, where = float(ratio.max()), name
        w = np_map_crf(trans, seq, viterbi=viterbi, dtype=np.float32)[0]
        assert (np.isnan(w) and np.isnan(res[0])) or np.float32(res[0]).tobytes() == np.float32(w).tobytes(), name
    print("float32, %s: worst ratio of |edits32 - f64| to its bound %.3f (%s)" % ("viterbi" if viterbi else "forward", worst, where))


def test_nan_patterns_of_the_hand_made_cases():
    """The restatement alone, on the cases whose answers are known by hand: it pins the definition's conventions (every insertion
    into an only path is NaN, the deletion of an only base is NaN, an all-zero matrix scores 0 in Viterbi), not the library --
    no code of the library runs here, and the test passes without the feature.  The library is held to these cases on the device:
    tests/test_gpu_crf_edits.py::test_hand_made_cases."""
    by = {n: (t, s) for n, t, s in CASES}
    base, sub, dele, ins = np_crf_edits(*by["only-path"])
    assert np.isfinite(base) and np.all(np.isnan(ins)) and np.all(np.isfinite(sub)) and np.all(np.isfinite(dele))
    base, sub, dele, ins = np_crf_edits(*by["L-equals-NB"])
    assert np.all(np.isfinite(ins)) and np.all(np.isfinite(sub))
    base, sub, dele, ins = np_crf_edits(*by["one-base"])
    assert sub.shape == (1, 4) and ins.shape == (2, 4) and np.isnan(dele).tolist() == [True] and np.all(np.isfinite(sub)) and np.all(np.isfinite(ins))
    base, sub, dele, ins = np_crf_edits(*by["one-base-one-block"])
    assert np.isfinite(base) and np.all(np.isfinite(ins)) and np.isnan(dele[0])      # two bases over two entries: the only path
    base, sub, dele, ins = np_crf_edits(*by["all-zero"])
    assert base == 0 and np.all(sub == 0) and np.all(dele == 0) and np.all(ins == 0)
    trans, seq = by["call-s2-n17"]
    res = np_crf_edits(trans, seq)
    for i, b in enumerate(seq):                                                      # the substitution that changes nothing: within rounding of base
        assert abs(float(res[1][i][b]) - float(res[0])) <= 1e-5 * max(1.0, abs(float(res[0]))), i


# ---------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------
def check_edits_plan(lens, nbs):
    """what the kernels rely on: a row holds cells 0 .. L and the spare slot, 16-byte starts, no two reads overlap"""
    pitch, rows, res, nrow, nres = sa.crf_edits_plan(lens, nbs)
    spans, rspans = [], []
    for k, (L, nb) in enumerate(zip(lens, nbs)):
        assert pitch[k] >= L + 2 and pitch[k] % 16 == 0 and pitch[k] == sa.lib().scrappie_hip_crf_edits_pitch(L)
        assert rows[k] % 4 == 0 and res[k] % 4 == 0
        size = 3 * (nb + 1) * int(pitch[k])
        assert size * 4 == sa.lib().scrappie_hip_crf_edits_row_bytes(L, nb)
        spans.append((int(rows[k]), int(rows[k]) + size))
        rspans.append((int(res[k]), int(res[k]) + 9 * L + 4))
    for sp, total in ((spans, nrow), (rspans, nres)):
        for (a0, a1), (b0, b1) in zip(sp, sp[1:]):
            assert a1 <= b0
        assert not sp or (sp[0][0] == 0 and sp[-1][1] <= total)
    return pitch, rows, res, nrow, nres


def test_plan_keeps_reads_apart():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 9, 40):
        check_edits_plan([int(x) for x in rng.integers(1, 800, n)], [int(x) for x in rng.integers(1, 900, n)])
    pitch, rows, res, nrow, nres = check_edits_plan([1, 14, 15, 730], [1, 5, 5, 800])
    assert pitch.tolist() == [16, 16, 32, 736] and rows.tolist() == [0, 96, 96 + 288, 96 + 288 + 576]
    assert res.tolist() == [0, 16, 16 + 132, 16 + 132 + 140] and nres == 16 + 132 + 140 + 6576 and nrow == 960 + 3 * 801 * 736
    assert sa.crf_edits_plan([], [])[3:] == (0, 0)
    with pytest.raises(ValueError):
        sa.crf_edits_plan([3, 4], [5])


def test_plan_under_sanitizers(tmp_path):
    """tests/crf_edits_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the plan on arrays of exactly n entries"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "crf_edits_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "crf_edits_asan.c"),
                        os.path.join(csrc, "sh_host.c"), "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]


def test_arguments_are_refused_before_any_launch():
    sigs = [np.zeros(1000, dtype=np.float32)] * 3
    f = sa.Engine.score_edits
    with pytest.raises(ValueError, match="per signal"):
        f(_NoEngine(), sigs, ["ACGT", "ACGA"])                                 # two sequences for three reads
    with pytest.raises(TypeError):
        sa.map_trans_edits(np.zeros((10, 25), dtype=np.float32), "ACGT")
    with pytest.raises(ValueError):
        sa.map_trans_edits(sa.ScrappyMatrix.from_numpy(np.zeros((4, 5), dtype=np.float32), sloika=False), "ACGT")


def test_edits_symbols_are_exported_and_declared():
    L = sa.lib()
    header = open(os.path.join(ROOT, "include", "scrappie_hip.h")).read()
    for nm in NEW_SYMBOLS:
        assert hasattr(L, nm), nm
        assert nm + "(" in header, nm
    for other in ("pyscrap_map.h", "pyscrap_raw.h"):
        assert "crf_edits" not in open(os.path.join(ROOT, "include", other)).read()
    forms = sa.crf_edits_form_counts()
    assert len(forms) == 12 and sum(1 for k in forms if k[0] == "rows") == 8 and sum(1 for k in forms if k[0] == "edits") == 4
    assert callable(sa.map_trans_edits) and callable(sa.apply_edit) and callable(sa.Engine.score_edits)
