"""Every single-base edit of a sequence scored against a flip-flop read INSIDE A BAND (the banded forms of k_crf_edits_rows and
k_crf_edits, csrc/sh_crf_edits.h), the part that needs no GPU.  np_crf_edits_banded is the definition (include/scrappie_hip.h states
it in words): np_crf_edits with F and G masked to the band of each entry and the new base's own cells free.  It is held here against
np_map_crf_masked -- np_map_crf with a boolean mask per cell instead of intervals -- on the edited sequence with the inherited mask:
in float64 to 1e-9, in float32 within the project's standing bound for re-associated sums.  Further: the full band is no band, base
is np_map_crf's banded score, the band around a path (scrappie_hip_map_crf_path_band), the row bytes and the layout of a banded
launch (under sanitizers through tests/crf_edits_band_asan.c), the Python argument checks and the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from test_crf_edits_cpu import CASES, all_edits, np_crf_edits, pick
from test_map_crf_cpu import BIG, _lse, map_crf_cases, no_path_band, np_bounds_sane, np_map_crf, path_bands
from test_map_multi_cpu import _NoEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scrappie_hip_map_crf_edits_banded_batch", "map_crf_edits_banded", "scrappie_hip_map_crf_path_band",
               "scrappie_hip_crf_edits_band_pitch", "scrappie_hip_crf_edits_band_row_bytes", "scrappie_hip_crf_edits_band_plan",
               "scrappie_hip_crf_edits_band_form_counts")
PATH_KINDS = ("around", "low-edge", "high-edge", "exact", "stall-slide")


# ---------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------
def band_mask(low, high, L):
    """(nblock + 1, L + 1) booleans: cell p of entry t is inside [low[t], high[t])"""
    p = np.arange(L + 1)[None, :]
    return (p >= np.asarray(low, dtype=np.int64)[:, None]) & (p < np.asarray(high, dtype=np.int64)[:, None])


def np_map_crf_masked_many(trans, seqs, masks, viterbi=True, dtype=np.float32):
    """np_map_crf's score of each of `seqs` (n, L) with `masks` (n, nblock + 1, L + 1): after an entry's row is complete every cell
    outside the mask is -1e30.  The sequences of a call run side by side; a cell's arithmetic is np_map_crf's, operand for operand.
    Returns n scores in `dtype`, NaN below -1e30 / 2."""
    tr_all = np.ascontiguousarray(trans, dtype=dtype)
    seqs = np.asarray(seqs, dtype=np.int64)
    masks = np.asarray(masks, dtype=bool)
    n, L = seqs.shape
    NB = tr_all.shape[0]
    assert masks.shape == (n, NB + 1, L + 1) and L >= 1 and NB >= 1
    big = dtype(BIG)
    b = np.zeros((n, L + 1), dtype=np.int64)
    b[:, 1:] = seqs
    bp = np.zeros((n, L + 1), dtype=np.int64)
    bp[:, 2:] = seqs[:, :-1]
    iBB, iBS, iSB = 5 * b + bp, 5 * b + 4, 20 + b
    B = np.full((n, L + 1), -big, dtype=dtype)
    S = B.copy()
    S[:, 0] = np.where(masks[:, 0, 0], dtype(0), -big)
    B[:, 1] = np.where(masks[:, 0, 1], dtype(0), -big)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(NB):
            tr = tr_all[t]
            nB = np.full((n, L + 1), -big, dtype=dtype)
            base = tr[iBB[:, 1:]] + B[:, :-1]
            stay = tr[iBS[:, 1:]] + S[:, :-1]
            v = np.where(stay > base, stay, base) if viterbi else _lse(base, stay)
            v[:, 0] = stay[:, 0]                            # B'[1] has the stay predecessor only
            nB[:, 1:] = v
            sb = tr[iSB] + B
            ss = tr[24] + S
            nS = np.where(ss > sb, ss, sb) if viterbi else _lse(sb, ss)
            nS[:, 0] = ss[:, 0]                             # S'[0] likewise
            m = masks[:, t + 1]
            B, S = np.where(m, nB, -big), np.where(m, nS, -big)
        xb, xs = B[:, L], S[:, L]
        score = np.where(xb >= xs, xb, xs) if viterbi else _lse(xb, xs)
    score = np.asarray(score, dtype=dtype)
    score[score < -big / 2] = np.nan
    return score


def np_map_crf_masked(trans, seq, mask, viterbi=True, dtype=np.float32):
    """np_map_crf with a boolean (nblock + 1, L + 1) mask instead of intervals: the score alone"""
    return np_map_crf_masked_many(trans, np.asarray(seq)[None, :], np.asarray(mask)[None], viterbi, dtype)[0]


def np_crf_edits_banded(trans, seq, low, high, viterbi=True, dtype=np.float32):
    """np_crf_edits (tests/test_crf_edits_cpu.py) inside the band [low[t], high[t]): F_B, F_S, G_B and G_S hold -1e30 at every cell
    outside the band of its entry, the new base's own cells X carry no band; everything else -- recursions, order, mx, the end rule,
    the NaN rule -- is np_crf_edits', line for line."""
    tr_all = np.ascontiguousarray(trans, dtype=dtype)
    seq = np.asarray(seq, dtype=np.int64)
    NB, L = tr_all.shape[0], len(seq)
    assert tr_all.shape[1] == 25 and NB >= 1 and L >= 1
    big = dtype(BIG)
    m = band_mask(low, high, L)
    assert m.shape == (NB + 1, L + 1)

    def mx(a, b):
        return np.where(b > a, b, a) if viterbi else _lse(a, b)

    def end(x, y):
        return np.where(x >= y, x, y) if viterbi else _lse(x, y)

    with np.errstate(over="ignore", invalid="ignore"):
        FB = np.full((NB + 1, L + 1), -big, dtype=dtype)
        FS = FB.copy()
        if m[0, 1]:
            FB[0, 1] = 0
        if m[0, 0]:
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
            v[0] = stay[0]
            FB[t + 1, 1:] = v
            v = mx(tr[20 + b] + FB[t], tr[24] + FS[t])
            v[0] = tr[24] + FS[t, 0]
            FS[t + 1] = v
            FB[t + 1, ~m[t + 1]] = -big                     # the band of entry t + 1
            FS[t + 1, ~m[t + 1]] = -big
        base = end(FB[NB, L], FS[NB, L])
        GB = np.full((NB + 1, L + 2), -big, dtype=dtype)
        GS = GB.copy()
        if m[NB, L]:
            GB[NB, L] = 0
            GS[NB, L] = 0
        nx = np.zeros(L + 1, dtype=np.int64)
        nx[:L] = seq
        for t in range(NB - 1, -1, -1):
            tr = tr_all[t]
            stB = tr[20 + b] + GS[t + 1, :L + 1]
            v = mx(tr[5 * nx + b] + GB[t + 1, 1:], stB)
            v[L] = stB[L]
            v[0] = -big
            v[~m[t]] = -big                                 # the band of entry t
            GB[t, :L + 1] = v
            stS = tr[24] + GS[t + 1, :L + 1]
            v = mx(tr[5 * nx + 4] + GB[t + 1, 1:], stS)
            v[L] = stS[L]
            v[~m[t]] = -big
            GS[t, :L + 1] = v
        i = np.arange(L + 1)
        hp = i >= 1
        pb = np.where(hp, seq[np.maximum(i - 1, 0)], 0)
        n0 = seq[np.minimum(i, L - 1)]
        n1 = seq[np.minimum(i + 1, L - 1)]
        G1 = GB[:, np.minimum(i + 1, L + 1)]
        G2 = GB[:, np.minimum(i + 2, L + 1)]
        XB = np.where(i == 0, dtype(0), -big)[None, :].repeat(4, axis=0).astype(dtype)      # the new base's cells: no band
        XS = np.full((4, L + 1), -big, dtype=dtype)
        sub = (-big + G2[0])[None, :].repeat(4, axis=0)
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
        closed = end(XB, XS)
        ins[:, L] = closed[:, L]
        sub[:, L - 1] = closed[:, L - 1]
        dele[L - 1] = end(FB[NB, L - 1], FS[NB, L - 1])
        if L == 1:
            dele[0] = np.nan
        out = [np.asarray(base, dtype=dtype).reshape(1), sub[:, :L].T.copy(), dele[:L].copy(), ins.T.copy()]
        for a in out:
            a[a < -big / 2] = np.nan
    return dtype(out[0][0]), out[1], out[2], out[3]


def edited_mask(mask, kind, i):
    """the mask of the edited sequence: every cell inherited from the original keeps its original cell's band -- the prefix's cells
    0 .. i their index, the suffix's theirs in the original --, the new base's cell (i + 1 of the edited sequence) is free"""
    free = np.ones((mask.shape[0], 1), dtype=bool)
    if kind == "sub":
        return np.concatenate([mask[:, :i + 1], free, mask[:, i + 2:]], axis=1)
    if kind == "ins":
        return np.concatenate([mask[:, :i + 1], free, mask[:, i + 1:]], axis=1)
    return np.concatenate([mask[:, :i + 1], mask[:, i + 2:]], axis=1)


def np_path_band(path, L, h):
    """scrappie_hip_map_crf_path_band restated"""
    cnt = np.asarray(path, dtype=np.int64) + 1
    lo = np.maximum(cnt - h, 0)
    lo[0] = 0
    hi = np.minimum(cnt + h + 1, L + 1)
    return lo.astype(np.uintp), hi.astype(np.uintp)


# ---------------------------------------------------------------------------
# the cases: CASES of test_crf_edits_cpu.py under every band
# ---------------------------------------------------------------------------
def bands_of(trans, seq):
    """[(name, low, high)] for a case: every path_bands kind around np_map_crf's own Viterbi path, the diagonal bands of half-width 1
    and 8, and no_path_band where the sequence is long enough for it"""
    NB, L = trans.shape[0], len(seq)
    out = []
    path = np_map_crf(trans, seq)[1]
    if path is not None:
        out += [(k,) + tuple(path_bands(path, L, k)) for k in PATH_KINDS]
    out += [("diagonal-%d" % h,) + tuple(sa.map_crf_diagonal_band(NB, L, h)) for h in (1, 8)]
    if L >= 3:
        out.append(("no-path",) + tuple(no_path_band(NB, L)))
    return [(k, lo, hi) for k, lo, hi in out if np_bounds_sane(lo, hi, NB, L)]


@pytest.fixture(scope="module")
def brute():
    """per case, band and form: the float64 and float32 scores of np_map_crf_masked on every edited sequence with the inherited mask,
    computed once (the edits of one kind have one length and run side by side)"""
    out = {}
    for name, trans, seq in CASES:
        edits = all_edits(seq)
        for bname, lo, hi in bands_of(trans, seq):
            mask = band_mask(lo, hi, len(seq))
            for vit in (True, False):
                f64, f32 = np.full(len(edits), np.nan), np.full(len(edits), np.nan)
                for kind in ("sub", "del", "ins"):
                    idx = [k for k, e in enumerate(edits) if e[0] == kind and len(seq) + (kind == "ins") - (kind == "del") >= 1]
                    if not idx:
                        continue
                    seqs = np.array([sa.apply_edit(seq, *edits[k]) for k in idx])
                    masks = np.array([edited_mask(mask, kind, edits[k][1]) for k in idx])
                    f64[idx] = np_map_crf_masked_many(trans, seqs, masks, vit, np.float64)
                    f32[idx] = np_map_crf_masked_many(trans, seqs, masks, vit, np.float32)
                out[name, bname, vit] = (f64, f32)
    return out


def test_the_cases_have_every_band():
    kinds = {}
    for name, trans, seq in CASES:
        for bname, lo, hi in bands_of(trans, seq):
            kinds[bname] = kinds.get(bname, 0) + 1
    print("bands over the cases: %r" % sorted(kinds.items()))
    assert set(kinds) == set(PATH_KINDS) | {"diagonal-1", "diagonal-8", "no-path"}
    assert all(kinds[k] == len(CASES) for k in PATH_KINDS + ("diagonal-1", "diagonal-8")) and kinds["no-path"] >= 10


# ---------------------------------------------------------------------------
# the mask restatement is np_map_crf
# ---------------------------------------------------------------------------
def test_mask_restatement_equals_np_map_crf():
    n = 0
    for c in map_crf_cases():
        trans, seq = c["trans"], c["seq"]
        NB, L = trans.shape[0], len(seq)
        bands = [("none", None, None)]
        path = np_map_crf(trans, seq)[1]
        if path is not None:
            bands += [(k,) + tuple(path_bands(path, L, k)) for k in PATH_KINDS]
        bands += [("diagonal-%d" % h,) + tuple(sa.map_crf_diagonal_band(NB, L, h)) for h in (1, 8)]
        if L >= 9 and NB >= 4 and 3 * NB >= L - 2:
            bands.append(("no-path",) + tuple(no_path_band(NB, L)))
        for bname, lo, hi in bands:
            mask = np.ones((NB + 1, L + 1), dtype=bool) if lo is None else band_mask(lo, hi, L)
            for vit in (True, False):
                for dt in (np.float32, np.float64):
                    want = np_map_crf(trans, seq, viterbi=vit, low=lo, high=hi, dtype=dt)[0]
                    got = np_map_crf_masked(trans, seq, mask, viterbi=vit, dtype=dt)
                    assert (np.isnan(want) and np.isnan(got)) or dt(got).tobytes() == dt(want).tobytes(), (c["name"], bname, vit, dt)
                    n += 1
    assert n > 800


# ---------------------------------------------------------------------------
# the definition against np_map_crf_masked of every edit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("viterbi", [True, False])
def test_float64_definition_equals_the_masked_dp_of_every_edit(brute, viterbi):
    worst, nans, total, blocked = 0.0, 0, 0, 0
    for name, trans, seq in CASES:
        for bname, lo, hi in bands_of(trans, seq):
            res = np_crf_edits_banded(trans, seq, lo, hi, viterbi=viterbi, dtype=np.float64)
            want = brute[name, bname, viterbi][0]
            got = np.array([pick(res, *e) for e in all_edits(seq)], dtype=np.float64)
            assert got.shape == want.shape == (9 * len(seq) + 4,)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (name, bname, np.flatnonzero(np.isnan(got) != np.isnan(want)))
            ok = ~np.isnan(want)
            nans += int(np.sum(~ok))
            total += len(want)
            err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
            if err.size:
                worst = max(worst, float(err.max()))
                assert err.max() <= 1e-9, (name, bname, float(err.max()))
            if bname == "no-path" and len(seq) >= 9 and trans.shape[0] >= 4:      # (as test_map_crf_cpu.py uses it: nothing gets through)
                assert np.isnan(res[0]) and np.all(np.isnan(got)), name
                blocked += 1
    print("float64, %s: worst relative difference to the masked DP of the edited sequence %.3g; %d of %d edits NaN"
          % ("viterbi" if viterbi else "forward", worst, nans, total))
    assert blocked >= 3


@pytest.mark.parametrize("viterbi", [True, False])
def test_float32_definition_within_the_standing_bound(brute, viterbi):
    """|edits32 - f64| <= 2 |np_map_crf_masked32(edited) - f64| + 1e-5 |f64|; the worst ratio of the left side to the right over all
    cases and bands, printed below: 0.192 (Viterbi), 0.352 (forward)"""
    worst, where = 0.0, None
    for name, trans, seq in CASES:
        for bname, lo, hi in bands_of(trans, seq):
            res = np_crf_edits_banded(trans, seq, lo, hi, viterbi=viterbi, dtype=np.float32)
            assert all(a.dtype == np.float32 for a in res[1:])
            f64, f32 = brute[name, bname, viterbi]
            got = np.array([pick(res, *e) for e in all_edits(seq)], dtype=np.float64)
            assert np.array_equal(np.isnan(got), np.isnan(f64)), (name, bname)
            ok = ~np.isnan(f64)
            lhs = np.abs(got[ok] - f64[ok])
            rhs = 2 * np.abs(f32[ok] - f64[ok]) + 1e-5 * np.abs(f64[ok])
            assert np.all(lhs <= rhs), (name, bname, float(np.max(lhs - rhs)))
            ratio = lhs / np.where(rhs > 0, rhs, 1.0)
            if ratio.size and ratio.max() > worst:
                worst, where = float(ratio.max()), (name, bname)
    print("float32, %s: worst ratio of |edits32 - f64| to its bound %.3f %r" % ("viterbi" if viterbi else "forward", worst, where))


def test_full_band_is_no_band_and_base_is_the_banded_score():
    for name, trans, seq in CASES:
        NB, L = trans.shape[0], len(seq)
        full = (np.zeros(NB + 1, dtype=np.uintp), np.full(NB + 1, L + 1, dtype=np.uintp))
        for vit in (True, False):
            for dt in (np.float32, np.float64):
                a = np_crf_edits(trans, seq, viterbi=vit, dtype=dt)
                b = np_crf_edits_banded(trans, seq, full[0], full[1], viterbi=vit, dtype=dt)
                for x, y in zip(a, b):
                    x, y = np.atleast_1d(np.asarray(x, dtype=dt)), np.atleast_1d(np.asarray(y, dtype=dt))
                    assert np.array_equal(np.isnan(x), np.isnan(y)) and x[~np.isnan(x)].tobytes() == y[~np.isnan(y)].tobytes(), (name, vit, dt)
                for bname, lo, hi in bands_of(trans, seq):
                    got = np_crf_edits_banded(trans, seq, lo, hi, viterbi=vit, dtype=dt)[0]
                    want = np_map_crf(trans, seq, viterbi=vit, low=lo, high=hi, dtype=dt)[0]
                    assert (np.isnan(want) and np.isnan(got)) or dt(got).tobytes() == dt(want).tobytes(), (name, bname, vit, dt)


def test_identity_substitution_may_exceed_base_and_a_tight_end_is_nan():
    """two consequences the header states, pinned on the restatement: in the band that is the Viterbi path alone the substitution that
    changes nothing is scored with its own cell free -- the forward score then sums over more paths than base, so it is never below base
    and somewhere above it (the Viterbi score cannot be: that band holds the best path) --; with low[nblock] == L the deletion of the last
    base closes on a cell outside the band"""
    by = {n: (t, s) for n, t, s in CASES}
    trans, seq = by["call-s2-n40"]
    L = len(seq)
    lo, hi = path_bands(np_map_crf(trans, seq)[1], L, "exact")
    base, sub, dele, ins = np_crf_edits_banded(trans, seq, lo, hi, viterbi=False, dtype=np.float64)
    same = np.array([sub[i][b] for i, b in enumerate(seq)])
    assert np.all(same >= base - 1e-9 * abs(base)) and np.any(same > base + 1e-6), (base, same)
    vbase, vsub = np_crf_edits_banded(trans, seq, lo, hi, viterbi=True, dtype=np.float64)[:2]
    assert np.all(np.abs(np.array([vsub[i][b] for i, b in enumerate(seq)]) - vbase) <= 1e-9 * abs(vbase))
    assert int(lo[-1]) == L and np.isnan(dele[L - 1]) and np.all(np.isfinite(sub[L - 1]))


# ---------------------------------------------------------------------------
# the band around a path
# ---------------------------------------------------------------------------
def test_path_band_is_valid_holds_the_path_and_equals_its_restatement():
    n = 0
    for c in map_crf_cases():
        trans, seq = c["trans"], c["seq"]
        NB, L = trans.shape[0], len(seq)
        path = np_map_crf(trans, seq)[1]
        if path is None:
            continue
        for h in (0, 1, 8, L + 3):
            lo, hi = sa.map_crf_path_band(path, L, h)
            assert lo.dtype == np.uintp and len(lo) == len(hi) == NB + 1
            assert np_bounds_sane(lo, hi, NB, L), (c["name"], h)
            cnt = path.astype(np.int64) + 1
            assert np.all(lo <= cnt) and np.all(cnt < hi), (c["name"], h)
            wlo, whi = np_path_band(path, L, h)
            assert np.array_equal(lo, wlo) and np.array_equal(hi, whi), (c["name"], h)
            if h > L:
                assert np.all(lo == 0) and np.all(hi == L + 1)
            n += 1
    assert n >= 4 * 30
    for path, L in (([0, 1], 2), ([-1, 0], 1), ([0, 0, 0], 1), ([-1, -1, 0, 1, 1, 2], 3)):      # the corners by hand
        for h in (0, 1, 5):
            lo, hi = sa.map_crf_path_band(path, L, h)
            assert np_bounds_sane(lo, hi, len(path) - 1, L), (path, h)
            assert np.array_equal(lo, np_path_band(path, L, h)[0]) and np.array_equal(hi, np_path_band(path, L, h)[1])


def test_path_band_refuses_what_is_no_path():
    good = [-1, 0, 0, 1, 2, 2]
    sa.map_crf_path_band(good, 3, 1)
    for bad, L in (([-1, 0, 0, 2, 2, 2], 3),        # a step of two
                   ([-1, 0, 1, 0, 1, 2], 3),        # a step down
                   ([-1, 0, 0, 1, 1, 1], 3),        # does not end with the last base
                   ([-1, 0, 1, 2, 3, 3], 3),        # beyond the sequence
                   ([-2, 0, 0, 1, 2, 2], 3),        # below -1
                   ([1, 1, 1, 2, 2, 2], 3),         # two bases through entry 0
                   ([2], 3)):                       # no block
        with pytest.raises(ValueError):
            sa.map_crf_path_band(bad, L, 1)
    with pytest.raises(ValueError):
        sa.map_crf_path_band(good, 0, 1)
    with pytest.raises(ValueError):
        sa.map_crf_path_band(good, 3, -1)
    sp, ip = C.POINTER(C.c_size_t), C.POINTER(C.c_int)
    p = np.array(good, dtype=np.int32)
    lo = np.zeros(6, dtype=np.uintp)
    f = sa.lib().scrappie_hip_map_crf_path_band
    assert f(None, 5, 3, 1, lo.ctypes.data_as(sp), lo.ctypes.data_as(sp)) == -1
    assert f(p.ctypes.data_as(ip), 5, 3, 1, None, lo.ctypes.data_as(sp)) == -1
    assert f(p.ctypes.data_as(ip), 5, 3, 1, lo.ctypes.data_as(sp), None) == -1


# ---------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------
def test_row_bytes():
    rng = np.random.default_rng(5)
    for NB, L, h in ((800, 712, 8), (800, 712, 32), (1, 1, 0), (17, 18, 1), (64, 10, 3), (300, 3262, 40)):
        lo, hi = sa.map_crf_diagonal_band(NB, L, h)
        w = int(np.max(hi.astype(np.int64) - lo.astype(np.int64)))
        rb = sa.crf_edits_band_row_bytes(lo, hi)
        assert rb <= 12 * (NB + 1) * (w + 32) and rb >= 12 * (NB + 1) * (w + 1), (NB, L, h)
        sp = C.POINTER(C.c_size_t)
        pitch = sa.lib().scrappie_hip_crf_edits_band_pitch(lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), NB)
        assert pitch % 16 == 0 and pitch >= w + 1 and rb == 12 * (NB + 1) * pitch
    lo, hi = sa.map_crf_diagonal_band(800, 712, 8)
    banded, full = sa.crf_edits_band_row_bytes(lo, hi), sa.lib().scrappie_hip_crf_edits_row_bytes(712, 800)
    print("800 blocks x 712 bases: %d row bytes in the diagonal band of half-width 8, %d without a band" % (banded, full))
    assert banded < full and banded == 12 * 801 * 32
    full_band = (np.zeros(801, dtype=np.uintp), np.full(801, 713, dtype=np.uintp))
    assert sa.crf_edits_band_row_bytes(*full_band) == full                   # 713 cells and the slot: the unbanded pitch
    with pytest.raises(ValueError):
        sa.crf_edits_band_row_bytes(lo, hi[:-1])


def check_band_plan(lens, bands):
    """what the banded kernels rely on: a row holds the widest entry's cells and one slot more, 16-byte starts, no two reads overlap"""
    pitch, rows, res, nrow, nres = sa.crf_edits_band_plan(lens, bands)
    spans, rspans = [], []
    for k, (L, (lo, hi)) in enumerate(zip(lens, bands)):
        w = int(np.max(np.asarray(hi, dtype=np.int64) - np.asarray(lo, dtype=np.int64)))
        nb = len(lo) - 1
        assert pitch[k] >= w + 1 and pitch[k] % 16 == 0 and pitch[k] <= w + 16
        assert rows[k] % 4 == 0 and res[k] % 4 == 0
        size = 3 * (nb + 1) * int(pitch[k])
        assert size * 4 == sa.crf_edits_band_row_bytes(lo, hi)
        spans.append((int(rows[k]), int(rows[k]) + size))
        rspans.append((int(res[k]), int(res[k]) + 9 * L + 4))
    for sp, total in ((spans, nrow), (rspans, nres)):
        for (a0, a1), (b0, b1) in zip(sp, sp[1:]):
            assert a1 <= b0
        assert not sp or (sp[0][0] == 0 and sp[-1][1] <= total)
    return pitch, rows, res, nrow, nres


def test_band_plan_keeps_reads_apart():
    rng = np.random.default_rng(4)
    for n in (0, 1, 2, 9, 30):
        nbs = [int(x) for x in rng.integers(1, 900, n)]
        lens = [int(rng.integers(1, nb + 2)) for nb in nbs]
        check_band_plan(lens, [sa.map_crf_diagonal_band(nb, L, int(rng.integers(0, 40))) for nb, L in zip(nbs, lens)])
    bands = [sa.map_crf_diagonal_band(5, 4, 0), sa.map_crf_diagonal_band(800, 712, 8), sa.map_crf_diagonal_band(800, 712, 32)]
    pitch, rows, res, nrow, nres = check_band_plan([4, 712, 712], bands)
    assert pitch.tolist() == [16, 32, 80] and rows.tolist() == [0, 288, 288 + 3 * 801 * 32] and nrow == 288 + 3 * 801 * (32 + 80)
    assert res.tolist() == [0, 40, 40 + 6412] and nres == 40 + 2 * 6412
    assert sa.crf_edits_band_plan([], [])[3:] == (0, 0)
    with pytest.raises(ValueError):
        sa.crf_edits_band_plan([3, 4], bands[:1])


def test_host_functions_under_sanitizers(tmp_path):
    """tests/crf_edits_band_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the path band, the row bytes and
    the banded plan on arrays of exactly nblock + 1 and exactly n entries"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "crf_edits_band_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "crf_edits_band_asan.c"),
                        os.path.join(csrc, "sh_host.c"), "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]


def test_arguments_are_refused_before_any_launch():
    sigs = [np.zeros(1000, dtype=np.float32)] * 3
    f = sa.Engine.score_edits
    with pytest.raises(ValueError, match="per signal"):
        f(_NoEngine(), sigs, ["ACGT", "ACGA"], bands=8)                         # two sequences for three reads
    with pytest.raises(ValueError, match="per signal"):
        f(_NoEngine(), sigs, "ACGT", bands=[8, None])                           # two bands for three reads
    assert sa.Engine._bands_per_read(8, 3) == [8, 8, 8]
    pair = (np.zeros(5, dtype=np.uintp), np.full(5, 4, dtype=np.uintp))
    assert all(b is not None and len(b) == 2 for b in sa.Engine._bands_per_read(pair, 3)) and len(sa.Engine._bands_per_read(pair, 3)) == 3
    assert sa.Engine._bands_per_read([pair, None], 2)[1] is None and sa.Engine._bands_per_read([pair, pair], 2)[0] is pair
    ragged = (pair[0], pair[1][:-1])                                            # two reads, a per-read pair whose edges differ in length: still per read
    got = sa.Engine._bands_per_read([ragged, pair], 2)
    assert got[0] is ragged and got[1] is pair
    assert sa.Engine._bands_per_read([list(pair[0]), list(pair[1])], 4)[3][1] == list(pair[1])      # plain lists as one pair for all reads
    m = sa.ScrappyMatrix.from_numpy(np.zeros((4, 25), dtype=np.float32), sloika=False)
    with pytest.raises(TypeError):
        sa.map_trans_edits(np.zeros((10, 25), dtype=np.float32), "ACGT", bands=2)
    with pytest.raises(ValueError):
        sa.map_trans_edits(m, "ACG", bands=(np.zeros(4), np.full(4, 4)))        # one entry per block only
    with pytest.raises(ValueError):
        sa.map_trans_edits(m, "ACG", bands=(np.ones(5), np.full(5, 4)))         # does not start at cell 0
    with pytest.raises(ValueError):
        sa.map_trans_edits(m, "ACG", bands=(np.zeros(5), np.full(5, 4), np.zeros(5)))


def test_band_symbols_are_exported_and_declared():
    L = sa.lib()
    header = open(os.path.join(ROOT, "include", "scrappie_hip.h")).read()
    for nm in NEW_SYMBOLS:
        assert hasattr(L, nm), nm
        assert nm + "(" in header, nm
    forms = sa.crf_edits_band_form_counts()
    assert len(forms) == 12 and sum(1 for k in forms if k[0] == "rows") == 8 and sum(1 for k in forms if k[0] == "edits") == 4
    assert callable(sa.map_crf_path_band) and callable(sa.crf_edits_band_plan) and callable(sa.crf_edits_band_row_bytes)
