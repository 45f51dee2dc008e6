"""Every single-base edit of a sequence scored against a transducer read INSIDE A BAND (the banded forms of k_map_edits_rows and
k_map_edits, csrc/sh_map_edits.h), the part that needs no GPU.  np_map_edits_band is the definition (include/scrappie_hip.h states it
in words): np_map_edits (tests/test_map_edits_cpu.py) with F and G masked to the band of each entry and the edit's own middle columns
free.  It is held here against np_map_masked -- np_map's unbanded recursion with a boolean mask per cell -- on every edited sequence
with the inherited mask: in float64 to 1e-9, in float32 within the project's standing bound for re-associated sums.  Further: the
full band is no band, a Viterbi band around the path keeps base, the band around a path (scrappie_hip_map_path_band), the row bytes
and the layout of a banded launch (under sanitizers through tests/map_edits_band_asan.c), the Python argument checks, the exports and
the CLI's refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from test_map_cpu import BIG, CLI, _lse, np_map
from test_map_edits_cpu import KMAX, PENS, all_edits, encode, flat, make_post, np_map_edits, same_bits
from test_map_multi_cpu import _NoEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scrappie_hip_map_edits_banded_batch", "map_post_edits_banded", "scrappie_hip_map_path_band", "scrappie_hip_map_edits_band_pitch",
               "scrappie_hip_map_edits_band_row_bytes", "scrappie_hip_map_edits_band_plan", "scrappie_hip_map_edits_band_form_counts",
               "scrappie_hip_map_edits_band_scratch")


# ---------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------
def band_mask(low, high, n):
    """(nblock, n) booleans: cell q of entry t + 1 is inside [low[t], high[t])"""
    q = np.arange(n)[None, :]
    return (q >= np.asarray(low, dtype=np.int64)[:, None]) & (q < np.asarray(high, dtype=np.int64)[:, None])


def np_bounds_sane(low, high, nblock, n):
    """are_bounds_sane restated"""
    lo, hi = np.asarray(low, dtype=np.int64), np.asarray(high, dtype=np.int64)
    if len(lo) != nblock or len(hi) != nblock or nblock == 0:
        return False
    ok = lo[0] == 0 and hi[-1] == n and np.all(lo <= n) and np.all(hi <= n) and np.all(lo <= hi)
    return bool(ok and np.all(lo[1:] <= hi[:-1]) and np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0))


def np_map_masked(post, states, pens, adm, viterbi=True, dtype=np.float32):
    """np_map's unbanded score of the state codes `states` where, once the row of entry t + 1 is complete, every cell outside
    adm[t] (nblock, len(states)) is -1e30; START and END carry no mask.  NaN below -1e30 / 2."""
    f = np.dtype(dtype).type
    post = np.asarray(post).astype(dtype)
    NB, n2 = post.shape[0], len(states)
    sp, kp, lpen = f(pens[0]), f(pens[1]), f(pens[2])
    big = f(BIG)
    mx = (lambda x, y: np.where(y > x, y, x)) if viterbi else _lse
    p = np.full(n2, -big, dtype=dtype)
    S, E = f(0), -big
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(NB):
            row = post[t]
            lps = row[-1]
            ls = mx(-lpen, lps)
            le = row[states]
            v = (p - sp) + lps
            if n2 > 1:
                v[1:] = mx(v[1:], p[:n2 - 1] + le[1:])
            if n2 > 2:
                v[2:] = mx(v[2:], (p[:n2 - 2] - kp) + le[2:])
            v[0] = mx(v[0], S + le[0])
            E = mx(E + ls, p[n2 - 1] - lpen)
            v[~adm[t]] = -big
            p, S = v.astype(dtype), S + ls
        score = float((np.fmax if viterbi else _lse)(p[n2 - 1], E))
    return score if score >= -float(BIG) / 2 else np.nan


def edit_shape(kind, i, n, k):
    """(n2, A, J, j0, Bn) of an edit as the definition numbers them"""
    if kind == "sub":
        n2, j0, A = n, min(i + 1, n), min(max(i - k + 1, 0), n)
    elif kind == "del":
        n2, j0, A = n - 1, min(i + 1, n), min(max(i - k + 1, 0), max(n - 1, 0))
    else:
        n2, j0, A = n + 1, min(i, n), min(max(i - k + 1, 0), n)
    Bn = n - j0
    J = n2 - Bn
    return n2, min(A, J), J, j0, Bn


def edited_mask(mask, kind, i, k):
    """the mask of the edited sequence: cells idx < A keep the band of the original cell idx, the suffix's cells that of their original
    index j0 + (idx - J), the M middle cells are free at every entry"""
    n2, A, J, j0, Bn = edit_shape(kind, i, mask.shape[1], k)
    adm = np.ones((mask.shape[0], n2), dtype=bool)
    adm[:, :A] = mask[:, :A]
    if Bn:
        adm[:, J:] = mask[:, j0:]
    return adm


def brute_edits_band(post, seq, k, pens, low, high, viterbi, dtype):
    """np_map_masked on every edited sequence with the inherited mask, as float64 values"""
    L = len(seq)
    mask = band_mask(low, high, L - k + 1)
    out = []
    for kind, i, c in all_edits(L):
        ed = sa.apply_edit(np.asarray(seq, dtype=np.int32), kind, i, c)
        out.append(np.nan if len(ed) < k else np_map_masked(post, encode(ed, k), pens, edited_mask(mask, kind, i, k), viterbi, dtype))
    return np.array(out, dtype=np.float64)


def np_map_edits_band(post, seq, k, pens, low, high, viterbi=True, dtype=np.float32):
    """np_map_edits (tests/test_map_edits_cpu.py) inside the band [low[t], high[t]) of nblock entries over the n = L - k + 1 states:
    F[t + 1] and G[t] (t >= 1) hold -1e30 at every cell outside the band of their entry -- entry t + 1 has band entry t --,
    G[NB][n - 1] = 0 only where that cell is admissible, the edit's own middle columns X carry no band; everything else -- recursions,
    order, mx, the end rule, the NaN rule -- is np_map_edits', line for line.  base is the end rule on the masked rows."""
    f = np.dtype(dtype).type
    post = np.ascontiguousarray(post).astype(dtype)
    seq = np.asarray(seq, dtype=np.int64)
    NB, nr = post.shape
    L = len(seq)
    assert nr == 4 ** k + 1 and NB >= 1 and 1 <= k <= KMAX
    sub = np.full((L, 4), np.nan, dtype=dtype)
    dele = np.full(L, np.nan, dtype=dtype)
    ins = np.full((L + 1, 4), np.nan, dtype=dtype)
    if L < k:
        return f(np.nan), sub, dele, ins
    n = L - k + 1
    m = band_mask(low, high, n)
    assert m.shape == (NB, n)
    s = encode(seq, k)
    STAY = nr - 1
    sp, kp, lpen = f(pens[0]), f(pens[1]), f(pens[2])
    big = f(BIG)

    def mx(a, b):
        return np.where(b > a, b, a) if viterbi else _lse(a, b)

    with np.errstate(over="ignore", invalid="ignore"):
        lps_all = post[:, STAY]
        ls_all = mx(np.full(NB, -lpen, dtype=dtype), lps_all)
        F = np.full((NB + 1, n), -big, dtype=dtype)
        FS = np.zeros(NB + 1, dtype=dtype)
        E = -big
        for t in range(NB):
            p, row, lps = F[t], post[t], lps_all[t]
            le = row[s]
            v = (p - sp) + lps
            if n > 1:
                v[1:] = mx(v[1:], p[:n - 1] + le[1:])
            if n > 2:
                v[2:] = mx(v[2:], (p[:n - 2] - kp) + le[2:])
            v[0] = mx(v[0], FS[t] + le[0])
            v[~m[t]] = -big                                 # the band of entry t + 1
            F[t + 1] = v
            FS[t + 1] = FS[t] + ls_all[t]
            E = mx(E + ls_all[t], p[n - 1] - lpen)
        base = (np.fmax if viterbi else _lse)(F[NB, n - 1], E)
        G = np.full((NB + 1, n), -big, dtype=dtype)
        if m[NB - 1, n - 1]:
            G[NB, n - 1] = 0
        GE = np.zeros(NB + 1, dtype=dtype)
        for t in range(NB - 1, -1, -1):
            row, lps, g = post[t], lps_all[t], G[t + 1]
            GE[t] = GE[t + 1] + ls_all[t]
            le = row[s]
            v = (lps - sp) + g
            if n > 1:
                v[:n - 1] = mx(v[:n - 1], le[1:] + g[1:])
            if n > 2:
                v[:n - 2] = mx(v[:n - 2], (le[2:] - kp) + g[2:])
            v[n - 1] = mx(v[n - 1], -lpen + GE[t + 1])
            if t >= 1:
                v[~m[t - 1]] = -big                         # the band of entry t (G[0] is never read)
            G[t] = v

        def edits(kind, c):
            I = np.arange(L + 1 if kind == "ins" else L)
            if kind == "sub":
                n2, j0, A = n, np.minimum(I + 1, n), np.clip(I - k + 1, 0, n)
            elif kind == "del":
                n2, j0, A = n - 1, np.minimum(I + 1, n), np.clip(I - k + 1, 0, max(n - 1, 0))
            else:
                n2, j0, A = n + 1, np.minimum(I, n), np.clip(I - k + 1, 0, n)
            Bn = n - j0
            A = np.minimum(A, n2 - Bn)
            J = n2 - Bn
            M = J - A
            assert np.all(M >= 0) and np.all(M <= k) and np.all(A >= 0)

            def base_at(p):
                cl = lambda q: seq[np.clip(q, 0, L - 1)]
                if kind == "sub":
                    return np.where(p == I, c, cl(p))
                if kind == "del":
                    return cl(np.where(p < I, p, p + 1))
                return np.where(p < I, cl(p), np.where(p == I, c, cl(p - 1)))

            mid = []
            for mm in range(KMAX):
                code = np.zeros(len(I), dtype=np.int64)
                for j in range(k):
                    code = code * 4 + base_at(A + mm + j)
                mid.append(code)
            s0, s1 = s[np.minimum(j0, n - 1)], s[np.minimum(j0 + 1, n - 1)]
            X = [np.full(len(I), -big, dtype=dtype) for _ in range(KMAX)]      # the edit's own columns: no band
            acc = np.full(len(I), -big, dtype=dtype)

            def ext_of(t):
                fa1 = np.where(A >= 1, F[t][np.maximum(A - 1, 0)], -big).astype(dtype)
                fa2 = np.where(A >= 2, F[t][np.maximum(A - 2, 0)], -big).astype(dtype)
                return [fa2, fa1] + X

            def pick(ext, at):
                out = ext[0].copy()
                for j in range(1, len(ext)):
                    out = np.where(at == j, ext[j], out)
                return out

            for t in range(NB):
                row, lps, ls = post[t], lps_all[t], ls_all[t]
                ext = ext_of(t)
                c1, c2 = pick(ext, M + 1), pick(ext, M)
                le0, le1 = row[s0], row[s1]
                g0, g1 = G[t + 1][np.minimum(j0, n - 1)], G[t + 1][np.minimum(j0 + 1, n - 1)]
                e = mx(acc + ls, c1 - lpen)
                y0 = np.where(J == 0, FS[t], c1) + le0
                y0 = np.where(J >= 2, mx(y0, (c2 - kp) + le0), y0)
                b = mx(acc, y0 + g0)
                b = np.where((Bn >= 2) & (J >= 1), mx(b, ((c1 - kp) + le1) + g1), b)
                acc = np.where(Bn == 0, e, b).astype(dtype)
                for mm in range(KMAX - 1, -1, -1):
                    q = A + mm
                    le = row[mid[mm] % (nr - 1)]
                    v = (X[mm] - sp) + lps
                    v = np.where(q >= 1, mx(v, ext[mm + 1] + le), v)
                    v = np.where(q >= 2, mx(v, (ext[mm] - kp) + le), v)
                    v = np.where(q == 0, mx(v, FS[t] + le), v)
                    X[mm] = np.where(mm < M, v, X[mm]).astype(dtype)
            last = pick(ext_of(NB), M + 1)
            closed = np.fmax(last, acc) if viterbi else _lse(last, acc)
            out = np.where(Bn == 0, closed, acc).astype(dtype)
            out[out < -big / 2] = np.nan
            if n2 < 1:
                out[:] = np.nan
            return out

        for c in range(4):
            sub[:, c] = edits("sub", c)
            ins[:, c] = edits("ins", c)
        dele[:] = edits("del", None)
    return f(base), sub, dele, ins


def np_path_band(path, n, h):
    """scrappie_hip_map_path_band restated"""
    p = np.asarray(path, dtype=np.int64).copy()
    at = np.flatnonzero(p >= 0)
    p[:at[0]] = 0
    p[at[-1] + 1:] = n - 1
    lo, hi = np.maximum(p - h, 0), np.minimum(p + h + 1, n)
    lo[0], hi[-1] = 0, n
    return lo.astype(np.uintp), hi.astype(np.uintp)


def full_band(NB, n):
    return np.zeros(NB, dtype=np.uintp), np.full(NB, n, dtype=np.uintp)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def unbanded_path(post, seq, k, pens):
    """np_map's unbanded Viterbi path of the sequence, or None where it never enters a state"""
    path = np_map(post, encode(seq, k), *pens, viterbi=True, dtype=np.float64)[1]
    return path if np.any(path >= 0) and path[path >= 0][0] == 0 and path[path >= 0][-1] == len(seq) - k else None


def band_cases():
    """(name, post, seq, k, pens, low, high, kind), fixed seeds: k = 1, 2, 3; L from k + 1 to 20; NB below, at and well above n; path
    bands of half-width 1, 2, 3 around the unbanded Viterbi path and diagonal bands (kind 'path' / 'diagonal': every edit finite on
    these), and the special bands by hand (kind 'special')"""
    out = []
    rng = np.random.default_rng(20261021)
    for k in (1, 2, 3):
        for L, NB in ((k + 1, 5), (k + 3, 2), (9, 9 - k + 1), (12, 19), (14, 30), (20, 11), (20, 45)):
            n = L - k + 1
            post, seq = make_post(NB, k, rng), rng.integers(0, 4, L).astype(np.int32)
            pens = PENS[(k + L + NB) % 2]
            path = unbanded_path(post, seq, k, pens)
            if path is not None:
                for h in (1, 2, 3):
                    lo, hi = np_path_band(path, n, h)
                    out.append(("k%d-L%d-nb%d-path%d" % (k, L, NB, h), post, seq, k, pens, lo, hi, "path"))
            if NB >= 2:
                lo, hi = sa.diagonal_bands(2 if NB >= n else 3, NB, n)
                lo[0], hi[-1] = 0, n
                out.append(("k%d-L%d-nb%d-diagonal" % (k, L, NB), post, seq, k, pens, lo, hi, "diagonal"))
    # the special bands: k = 2, L = 9 (n = 8), NB = 12
    k, L, NB = 2, 9, 12
    n = L - k + 1
    post, seq = make_post(NB, k, rng), rng.integers(0, 4, L).astype(np.int32)
    sp = lambda name, lo, hi: out.append((name, post, seq, k, PENS[1], np.array(lo, dtype=np.uintp), np.array(hi, dtype=np.uintp), "special"))
    sp("empty-entry", [0, 0, 1, 2, 3, 5, 5, 5, 5, 6, 6, 7], [2, 3, 4, 5, 5, 5, 6, 7, 8, 8, 8, 8])              # low[5] == high[5]: nothing gets through
    sp("low-last-is-n", [0, 0, 1, 2, 3, 4, 5, 6, 6, 7, 7, 8], [2, 3, 4, 5, 6, 7, 8, 8, 8, 8, 8, 8])            # low[NB - 1] == n
    sp("start-in-block-0-only", [0, 1, 1, 2, 3, 4, 4, 5, 5, 6, 6, 7], [1, 3, 4, 5, 6, 7, 7, 8, 8, 8, 8, 8])    # low[1] > 0
    sp("tight-ends", [0, 2, 2, 3, 3, 5, 5, 5, 6, 6, 6, 8], [2, 4, 4, 5, 5, 7, 7, 7, 8, 8, 8, 8])               # two cells per entry, low[1] == 2, low[NB - 1] == n
    return out


CASES = band_cases()


@pytest.fixture(scope="module")
def brute():
    """per case and form: np_map_masked on every edited sequence in float64 and float32, computed once"""
    out = {}
    for name, post, seq, k, pens, lo, hi, kind in CASES:
        for vit in (True, False):
            out[name, vit] = (brute_edits_band(post, seq, k, pens, lo, hi, vit, np.float64), brute_edits_band(post, seq, k, pens, lo, hi, vit, np.float32))
    return out


def test_the_cases_are_valid_bands_of_every_kind():
    kinds = {}
    for name, post, seq, k, pens, lo, hi, kind in CASES:
        NB, n = post.shape[0], len(seq) - k + 1
        assert np_bounds_sane(lo, hi, NB, n), name
        sp = C.POINTER(C.c_size_t)
        assert sa.lib().are_bounds_sane(lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), NB, n), name
        kinds[kind] = kinds.get(kind, 0) + 1
    by = {c[0]: c for c in CASES}
    lo, hi = by["empty-entry"][5:7]
    assert np.any(lo == hi)
    assert int(by["low-last-is-n"][5][-1]) == 8 and int(by["start-in-block-0-only"][5][1]) > 0
    assert kinds["path"] >= 40 and kinds["diagonal"] >= 15 and kinds["special"] == 4, kinds
    ks = {c[3] for c in CASES}
    assert ks == {1, 2, 3}
    shapes = {(c[1].shape[0], len(c[2]) - c[3] + 1) for c in CASES}
    assert any(nb < n for nb, n in shapes) and any(nb == n for nb, n in shapes) and any(nb >= 2 * n for nb, n in shapes)


# ---------------------------------------------------------------------------
# the definition against the masked DP of every edit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("viterbi", [True, False])
def test_float64_definition_equals_the_masked_dp_of_every_edit(brute, viterbi):
    worst, finite, nans = 0.0, 0, 0
    for name, post, seq, k, pens, lo, hi, kind in CASES:
        res = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=viterbi, dtype=np.float64)
        want = brute[name, viterbi][0]
        got = flat(res, len(seq))
        assert got.shape == want.shape == (9 * len(seq) + 4,)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, np.flatnonzero(np.isnan(got) != np.isnan(want)))
        ok = ~np.isnan(want)
        if kind != "special":
            finite += int(ok.sum())
        nans += int((~ok).sum())
        err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
        if err.size:
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-9, (name, float(err.max()))
    assert finite > 1000
    print("float64, %s: %d finite edits in path and diagonal bands, %d NaN over all cases, worst relative difference to the masked DP of the "
          "edited sequence %.3g" % ("viterbi" if viterbi else "forward", finite, nans, worst))


@pytest.mark.parametrize("viterbi", [True, False])
def test_float32_definition_within_the_standing_bound(brute, viterbi):
    """|edits32 - f64| <= 2 |np_map_masked32(edited) - f64| + 1e-5 |f64|; the worst ratio of the left side to the right is printed"""
    worst, where = 0.0, None
    for name, post, seq, k, pens, lo, hi, kind in CASES:
        res = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=viterbi, dtype=np.float32)
        assert all(a.dtype == np.float32 for a in res[1:])
        f64, f32 = brute[name, viterbi]
        got = flat(res, len(seq))
        assert np.array_equal(np.isnan(got), np.isnan(f64)), name
        ok = ~np.isnan(f64)
        lhs = np.abs(got[ok] - f64[ok])
        rhs = 2 * np.abs(f32[ok] - f64[ok]) + 1e-5 * np.abs(f64[ok])
        ratio = lhs / np.where(rhs > 0, rhs, 1.0)
        if ratio.size and ratio.max() > worst:
            worst, where = float(ratio.max()), name
        assert np.all(lhs <= rhs), (name, float(np.max(lhs - rhs)))
    print("float32, %s: worst ratio of |edits32 - f64| to its bound %.3f (%s)" % ("viterbi" if viterbi else "forward", worst, where))


def test_full_band_is_no_band():
    """the bits of np_map_edits, all outputs, both forms, both precisions"""
    seen = set()
    for name, post, seq, k, pens, lo, hi, kind in CASES:
        if id(post) in seen:
            continue
        seen.add(id(post))
        fl, fh = full_band(post.shape[0], len(seq) - k + 1)
        for vit in (True, False):
            for dt in (np.float32, np.float64):
                a = np_map_edits(post, seq, k, pens, viterbi=vit, dtype=dt)
                b = np_map_edits_band(post, seq, k, pens, fl, fh, viterbi=vit, dtype=dt)
                for x, y in zip(a, b):
                    x, y = np.atleast_1d(np.asarray(x, dtype=dt)), np.atleast_1d(np.asarray(y, dtype=dt))
                    assert np.array_equal(np.isnan(x), np.isnan(y)) and x[~np.isnan(x)].tobytes() == y[~np.isnan(y)].tobytes(), (name, vit, dt)
    assert len(seen) >= 20


def test_a_viterbi_band_around_the_path_keeps_base():
    """float64, whose path the bands are built around (float32's own path may differ where two paths tie to rounding)"""
    n = 0
    for name, post, seq, k, pens, lo, hi, kind in CASES:
        if kind != "path":
            continue
        got = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=True, dtype=np.float64)[0]
        want = np_map_edits(post, seq, k, pens, viterbi=True, dtype=np.float64)[0]
        assert same_bits(got, want, np.float64), name
        n += 1
    assert n >= 40


def test_base_is_not_the_reference_banded_score_and_identity_may_exceed_base_and_tight_ends_are_nan():
    """three consequences the header states, pinned on the restatement"""
    by = {c[0]: c for c in CASES}
    name, post, seq, k, pens, lo, hi, kind = by["tight-ends"]
    L, n = len(seq), len(seq) - k + 1
    base, sub, dele, ins = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=False, dtype=np.float64)
    got = flat((base, sub, dele, ins), L)
    nan_at = set(np.flatnonzero(np.isnan(sub).any(axis=1))) | set(np.flatnonzero(np.isnan(dele))) | set(np.flatnonzero(np.isnan(ins).any(axis=1)))
    assert nan_at and all(i <= 1 or i >= L - 1 for i in nan_at), nan_at        # edits at an end without a path: a result, not an error
    assert np.isfinite(base) and np.sum(np.isfinite(got)) > len(got) // 2
    # the reference's banded recursion (np_map with low / high) keeps stale cells: on some case its score is another number
    differs = 0
    for name, post, seq, k, pens, lo, hi, kind in CASES:
        if len(seq) - k + 1 < 3:
            continue
        ref = np_map(post, encode(seq, k), *pens, viterbi=True, low=lo, high=hi, dtype=np.float64)[0]
        mine = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=True, dtype=np.float64)[0]
        differs += int(not (np.isnan(mine) and np.isnan(ref)) and float(ref) != float(mine))
    assert differs >= 1
    # identity substitution, forward, in the band that is the path and one state to either side: never below base, somewhere above
    name, post, seq, k, pens, lo, hi, kind = by["k2-L12-nb19-path1"]
    base, sub, dele, ins = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=False, dtype=np.float64)
    same = np.array([sub[i][b] for i, b in enumerate(seq)])
    assert np.all(same >= base - 1e-9 * abs(base)) and np.any(same > base + 1e-6), (base, same)


# ---------------------------------------------------------------------------
# the band around a path
# ---------------------------------------------------------------------------
def random_path(n, NB, lead, trail, rng):
    """a path of NB blocks over n states: `lead` -1s, position 0 .. n - 1 in steps of 0, 1 or 2, `trail` -1s"""
    body = NB - lead - trail
    assert body >= (n + 1) // 2 and body >= 1
    while True:
        steps = rng.integers(0, 3, body - 1) if body > 1 else np.zeros(0, dtype=np.int64)
        pos = np.concatenate([[0], np.cumsum(steps)])
        if pos[-1] >= n - 1:
            break
    pos = np.minimum(pos, n - 1)
    # trim the overshoot into a legal tail: stay at n - 1 once reached
    return np.concatenate([np.full(lead, -1), pos, np.full(trail, -1)]).astype(np.int32)


def test_path_band_is_valid_holds_the_path_and_equals_its_restatement():
    rng = np.random.default_rng(11)
    cnt, skips = 0, 0
    for n, NB, lead, trail in ((1, 1, 0, 0), (1, 4, 2, 1), (2, 3, 0, 1), (8, 12, 0, 0), (8, 12, 3, 2), (30, 40, 5, 0), (30, 25, 0, 4), (257, 300, 7, 9)):
        for rep in range(4):
            path = random_path(n, NB, lead, trail, rng)
            body = path[path >= 0]
            skips += int(np.sum(np.diff(body) == 2))
            for h in range(1, 9):
                lo, hi = sa.map_path_band(path, n, h)
                assert lo.dtype == np.uintp and len(lo) == len(hi) == NB
                assert np_bounds_sane(lo, hi, NB, n), (n, NB, h)
                sp = C.POINTER(C.c_size_t)
                assert sa.lib().are_bounds_sane(lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), NB, n)
                at = path >= 0
                assert np.all(lo[at] <= path[at]) and np.all(path[at] < hi[at]), (n, NB, h)
                wlo, whi = np_path_band(path, n, h)
                assert np.array_equal(lo, wlo) and np.array_equal(hi, whi), (n, NB, h)
                cnt += 1
    assert cnt == 8 * 4 * 8 and skips > 20
    for name, post, seq, k, pens, lo, hi, kind in CASES:      # np_map's own paths
        if kind == "path":
            path = unbanded_path(post, seq, k, pens)
            h = int(name[-1])
            got = sa.map_path_band(path, len(seq) - k + 1, h)
            assert np.array_equal(got[0], lo) and np.array_equal(got[1], hi), name


def test_path_band_refuses_what_is_no_path():
    good = [-1, 0, 0, 1, 3, 3, -1]
    sa.map_path_band(good, 4, 1)
    with pytest.raises(ValueError):
        sa.map_path_band(good, 4, 0)                        # a half-width of 0 cannot hold a skip
    for bad, n in (([-1, 0, 0, 1, 4, 4, -1], 4),            # beyond the sequence
                   ([-2, 0, 0, 1, 3, 3, -1], 4),            # below -1
                   ([-1, 0, 1, 0, 3, 3, -1], 4),            # a step down
                   ([-1, 0, 0, 3, 3, 3, -1], 4),            # a step of three
                   ([-1, 0, 1, -1, 3, 3, -1], 4),           # a -1 between positions
                   ([-1, -1, -1, -1], 4),                   # no position at all
                   ([-1, 1, 2, 3, 3, -1], 4),               # a first position other than 0
                   ([-1, 0, 1, 2, 2, -1], 4)):              # a last other than nstate - 1
        with pytest.raises(ValueError):
            sa.map_path_band(bad, n, 2)
    with pytest.raises(ValueError):
        sa.map_path_band(good, 0, 1)
    with pytest.raises(ValueError):
        sa.map_path_band([], 4, 1)
    sp, ip = C.POINTER(C.c_size_t), C.POINTER(C.c_int)
    p = np.array(good, dtype=np.int32)
    lo = np.zeros(7, dtype=np.uintp)
    f = sa.lib().scrappie_hip_map_path_band
    assert f(None, 7, 4, 1, lo.ctypes.data_as(sp), lo.ctypes.data_as(sp)) == -1
    assert f(p.ctypes.data_as(ip), 7, 4, 1, None, lo.ctypes.data_as(sp)) == -1
    assert f(p.ctypes.data_as(ip), 7, 4, 1, lo.ctypes.data_as(sp), None) == -1
    assert f(p.ctypes.data_as(ip), 0, 4, 1, lo.ctypes.data_as(sp), lo.ctypes.data_as(sp)) == -1
    assert f(p.ctypes.data_as(ip), 7, 4, 0, lo.ctypes.data_as(sp), lo.ctypes.data_as(sp)) == -1


# ---------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------
def diag(NB, n, h):
    lo, hi = sa.diagonal_bands(h, NB, n)
    lo[0], hi[-1] = 0, n
    return lo, hi


def test_row_bytes():
    for NB, n, h in ((800, 726, 8), (800, 726, 32), (1, 1, 1), (17, 18, 1), (64, 10, 3), (300, 3262, 40)):
        lo, hi = diag(NB, n, h)
        w = int(np.max(hi.astype(np.int64) - lo.astype(np.int64)))
        rb = sa.map_edits_band_row_bytes(lo, hi)
        sp = C.POINTER(C.c_size_t)
        pitch = sa.lib().scrappie_hip_map_edits_band_pitch(lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), NB)
        assert pitch % 16 == 0 and pitch >= w + 1 and pitch <= w + 16 and rb == 8 * (NB + 1) * pitch, (NB, n, h)
    lo, hi = diag(800, 726, 8)
    banded, full = sa.map_edits_band_row_bytes(lo, hi), sa.lib().scrappie_hip_map_edits_row_bytes(730, 5, 800)
    print("800 blocks x 730 bases (k = 5): %d row bytes in the diagonal band of 8, %d without a band" % (banded, full))
    assert banded < full // 10
    assert sa.map_edits_band_row_bytes(*full_band(800, 726)) == full          # 726 cells and the slot: the unbanded pitch
    with pytest.raises(ValueError):
        sa.map_edits_band_row_bytes(lo, hi[:-1])
    assert sa.lib().scrappie_hip_map_edits_band_pitch(None, None, 5) == 0


def check_band_plan(lens, bands, k):
    """what the banded kernels rely on: a row holds the widest entry's cells and its slot, 16-byte starts, no two reads overlap; a read
    without a band takes the unbanded pitch"""
    pitch, rows, res, nrow, nres = sa.map_edits_band_plan(lens, bands, k)
    spans, rspans = [], []
    for j, (L, (lo, hi)) in enumerate(zip(lens, bands)):
        if hi is None:
            nb = int(lo)
            assert pitch[j] == sa.lib().scrappie_hip_map_edits_pitch(L, k)
        else:
            w = int(np.max(np.asarray(hi, dtype=np.int64) - np.asarray(lo, dtype=np.int64)))
            nb = len(lo)
            assert pitch[j] >= w + 1 and pitch[j] % 16 == 0 and pitch[j] <= w + 16
            assert 2 * (nb + 1) * int(pitch[j]) * 4 == sa.map_edits_band_row_bytes(lo, hi)
        assert rows[j] % 4 == 0 and res[j] % 4 == 0
        size = 2 * (nb + 1) * int(pitch[j])
        spans.append((int(rows[j]), int(rows[j]) + size))
        rspans.append((int(res[j]), int(res[j]) + 9 * L + 4))
    for sp, total in ((spans, nrow), (rspans, nres)):
        for (a0, a1), (b0, b1) in zip(sp, sp[1:]):
            assert a1 <= b0
        assert not sp or (sp[0][0] == 0 and sp[-1][1] <= total)
    return pitch, rows, res, nrow, nres


def test_band_plan_keeps_reads_apart():
    rng = np.random.default_rng(4)
    for k in (1, 3, 5):
        for cnt in (0, 1, 2, 9, 30):
            nbs = [int(x) for x in rng.integers(2, 900, cnt)]
            lens = [int(rng.integers(k, 700)) for nb in nbs]
            bands = [(nb, None) if rng.integers(0, 4) == 0 else diag(nb, L - k + 1, int(rng.integers(1, 40))) for nb, L in zip(nbs, lens)]
            check_band_plan(lens, bands, k)
    bands = [diag(5, 4, 1), diag(800, 726, 8), (800, None), diag(800, 726, 32)]
    pitch, rows, res, nrow, nres = check_band_plan([8, 730, 730, 730], bands, 5)
    assert pitch.tolist()[2] == 736 and pitch[1] < pitch[3] < 736
    assert rows.tolist()[:2] == [0, 2 * 6 * int(pitch[0])] and nrow == int(rows[3]) + 2 * 801 * int(pitch[3])
    assert sa.map_edits_band_plan([], [], 5)[3:] == (0, 0)
    with pytest.raises(ValueError):
        sa.map_edits_band_plan([30, 40], bands[:1], 5)
    with pytest.raises(ValueError):
        sa.map_edits_band_plan([3], [diag(5, 4, 1)], 5)     # fewer bases than a k-mer


def test_host_functions_under_sanitizers(tmp_path):
    """tests/map_edits_band_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the path band, the row bytes and the
    banded plan on arrays of exactly nblock and exactly n entries"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "map_edits_band_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "map_edits_band_asan.c"),
                        os.path.join(csrc, "sh_host.c"), "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]


def test_arguments_are_refused_before_any_launch():
    sigs = [np.zeros(1000, dtype=np.float32)] * 3
    f = sa.Engine.score_edits_transducer
    with pytest.raises(ValueError, match="per signal"):
        f(_NoEngine(), sigs, ["ACGTACGT", "ACGAACGT"], bands=8)                 # two sequences for three reads
    with pytest.raises(ValueError, match="per signal"):
        f(_NoEngine(), sigs, "ACGTACGT", bands=[8, None])                       # two bands for three reads
    m = sa.ScrappyMatrix.from_numpy(np.zeros((6, 17), dtype=np.float32), sloika=False)
    with pytest.raises(TypeError):
        sa.map_post_edits(np.zeros((10, 17), dtype=np.float32), "ACGT", bands=2)
    with pytest.raises(ValueError):
        sa.map_post_edits(m, "ACGTA", bands=(np.zeros(7), np.full(7, 4)))       # one entry per block only
    with pytest.raises(ValueError):
        sa.map_post_edits(m, "ACGTA", bands=(np.ones(6), np.full(6, 4)))        # does not start at state 0
    with pytest.raises(ValueError):
        sa.map_post_edits(m, "ACGTA", bands=(np.zeros(6), np.full(6, 4), np.zeros(6)))
    # the C calls: a null band, one edge alone -- before any device is touched
    fp, sp, ip = C.POINTER(C.c_float), C.POINTER(C.c_size_t), C.POINTER(C.c_int)
    seq = np.array([0, 1, 2, 3, 0], dtype=np.int32)
    lo = np.zeros(6, dtype=np.uintp)
    base = C.c_float(0.0)
    assert sa.lib().map_post_edits_banded(m.data(), 0.0, 0.0, 4.0, seq.ctypes.data_as(ip), 5, None, lo.ctypes.data_as(sp), 1, C.byref(base), None, None, None) == -1
    assert np.isnan(base.value) and "null argument" in sa.last_error()
    assert sa.lib().map_post_edits_banded(m.data(), 0.0, 0.0, 4.0, seq.ctypes.data_as(ip), 5, lo.ctypes.data_as(sp), None, 1, C.byref(base), None, None, None) == -1


def test_band_symbols_are_exported_and_declared():
    L = sa.lib()
    header = open(os.path.join(ROOT, "include", "scrappie_hip.h")).read()
    for nm in NEW_SYMBOLS:
        assert hasattr(L, nm), nm
        assert nm + "(" in header, nm
    forms = sa.map_edits_band_form_counts()
    assert len(forms) == 16 and sum(1 for q in forms if q[0] == "rows") == 8
    assert sum(1 for q in forms if q[0] == "edits" and q[3] == 64) == 4 and sum(1 for q in forms if q[0] == "edits" and q[3] == 256) == 4
    assert callable(sa.map_path_band) and callable(sa.map_edits_band_plan) and callable(sa.map_edits_band_row_bytes) and callable(sa.map_edits_band_scratch)
    assert "with these changes and no other" in header and "NOT map_to_sequence_viterbi_banded" in header


def test_seqmappy_kmer_edits_band_without_gpu(tmp_path):
    """--help names the combination; the refusals that need no device"""
    h = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    text = h.stdout + h.stderr
    assert "--band" in text and "--kmer-edits --band" in text
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTAC\n")
    r = subprocess.run([CLI, "seqmappy", "--kmer-edits", "--band", "0", str(fa), "nothing.fast5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == "" and "--band" in r.stderr and "skip moves two states" in r.stderr, r.stderr
    r = subprocess.run([CLI, "seqmappy", "--band", "8", str(fa), "nothing.fast5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == "" and "--band" in r.stderr and "--edits" in r.stderr, r.stderr
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--kmer-edits", "--band", "8", str(fa), "nothing.fast5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == "" and "(--edits)" in r.stderr, r.stderr
