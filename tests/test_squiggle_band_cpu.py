"""Banded squiggle matching (sh_squig_band.h) without a GPU.

`np_squiggle_match_banded` is `np_squiggle_match` of tests/test_squiggle_cpu.py with the band's one change: once the row of
sample t is complete (emission added), every position state and every back state whose position lies outside
[low[t], min(low[t] + width, npos)) holds -1e30; START and END are never masked.  Held here against the unbanded restatement
and the reference's compiled code: the full band and every band that contains the reference's path give the reference's score
and path bit for bit.  Also here: the diagonal helper against its formula, the band's argument errors (NAN and a text, nothing
launched), and the banded planner's layout.  tests/test_gpu_squiggle_band.py holds the GPU against this restatement."""
import ctypes as C

import numpy as np
import pytest

import oracle
import scrappie_amd as sa
from scrappie_amd import synth
from test_squiggle_cpu import (BIG, M_LN2, PENS, _lse, _tables, call_squig, lds_threshold, np_squiggle_match, ref_squiggle_lib,
                               squig_cases, squig_scratch_cases)


def np_squiggle_match_banded(low, width, signal, params, rate, prob_back, local_pen, skip_pen, minscore, viterbi=True, dtype=np.float32):
    """np_squiggle_match inside the band (low[t] per sample, width): (score, path or None); a score below -1e29: no path"""
    f = np.dtype(dtype).type
    x = np.asarray(signal, dtype=np.float32).astype(dtype)
    par = np.ascontiguousarray(params, dtype=np.float32)
    NP, ns = len(par), len(x)
    NF = NP + 2
    NST = NF + NP
    low = np.asarray(low, dtype=np.int64)
    assert len(low) == ns and width >= 1 and np.all(low >= 0) and np.all(low <= NP - 1) and np.all(np.diff(low) >= 0)
    positions = np.arange(NP)
    with np.errstate(all="ignore"):
        loc, logsc, scale, move, stay, back_pen, half = _tables(par, rate, prob_back, dtype)
        loc, logsc, scale = loc.astype(dtype), logsc.astype(dtype), scale.astype(dtype)
        lp, kp, ms = f(np.float32(local_pen)), f(np.float32(skip_pen)), f(np.float32(minscore))
        dest = np.arange(1, NP).astype(dtype)
        delta = (NP - np.arange(1, NP)).astype(dtype)
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
                    k = int(np.argmax(cand))
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
                if NP > 1:
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
            out = (positions < low[t]) | (positions >= low[t] + width)          # the band's one change
            c[1:NP + 1][out] = -f(BIG)
            c[NF:][out] = -f(BIG)
        if not viterbi:
            return _lse(c[NF - 2], c[NF - 1]), None
        score = np.fmax(c[NF - 2], c[NF - 1])
    if score < -1e29:
        return score, None
    path = np.zeros(ns, dtype=np.int64)
    path[-1] = NF - 2 if c[NF - 2] > c[NF - 1] else NF - 1
    for t in range(ns - 1, 0, -1):
        path[t - 1] = tb[t, path[t]]
    lo, hi = 0, ns
    while lo < ns and path[lo] == 0:
        path[lo] = -1; lo += 1
    while hi > 0 and path[hi - 1] == NF - 1:
        path[hi - 1] = -1; hi -= 1
    for t in range(lo, hi):
        assert path[t] > 0
        path[t] -= NF if path[t] >= NF else 1
    return score, path.astype(np.int32)


# ---------------------------------------------------------------------------
# bands made from a path
# ---------------------------------------------------------------------------
def path_envelope(path, npos):
    """(lo, hi), both non-decreasing, with lo[t] <= path[t] <= hi[t] wherever the path is mapped: hi the running maximum of the
    mapped positions so far, lo the minimum of those still to come; samples in START / END (-1) take their neighbours' values"""
    path = np.asarray(path, dtype=np.int64)
    ns = len(path)
    hi = np.maximum.accumulate(np.where(path >= 0, path, 0))
    lo = np.minimum.accumulate(np.where(path >= 0, path, npos - 1)[::-1])[::-1]
    lo = np.minimum(lo, hi)
    assert len(lo) == ns and np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0)
    return lo, hi


def hugging_band(path, npos, margin):
    """(low, width): the narrowest band of one width around the path's monotone envelope, `margin` positions wider on each side"""
    lo, hi = path_envelope(path, npos)
    width = int(min(npos, np.max(hi - lo) + 1 + 2 * margin))
    low = np.clip(lo - margin, 0, npos - 1)
    return low.astype(np.int32), width


def band_contains(path, low, width):
    path = np.asarray(path)
    m = path >= 0
    return bool(np.all((path[m] >= low[m]) & (path[m] < low[m].astype(np.int64) + width)))


def small_cases():
    """the inputs of squig_cases and squig_scratch_cases whose restatement runs in a fraction of a second"""
    T = lds_threshold()
    return [c for c in squig_cases(T) + squig_scratch_cases(T) if len(c[4]) * (c[3] - c[2]) <= 70000]


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_small_cases_cover_the_penalties_and_a_window():
    cases = small_cases()
    assert len(cases) >= 20 and {c[5] for c in cases} == set(PENS)
    assert any(c[2] > 0 and c[3] < len(c[1]) for c in cases)
    assert any(len(c[4]) > lds_threshold() for c in cases) and any(len(c[4]) == 1 for c in cases)


def test_full_band_and_bands_around_the_path_equal_the_reference():
    """the full band, and hugging bands of margins 0, 1 and 5 around the reference's path: the reference's score and path bit
    for bit; the full band equals the unbanded restatement in forward too"""
    R = ref_squiggle_lib()
    if R is None:
        pytest.skip("oracle/_ref/libref_decode.so not built")
    nbands = 0
    for name, sig, start, end, params, pens in small_cases():
        npos, ns = len(params), end - start
        want_s, want_p = call_squig(R, sig, start, end, params, pens, True)
        win = want_p[start:end]
        un_s, un_p = np_squiggle_match(sig[start:end], params, *pens, viterbi=True)
        assert np.float32(un_s).tobytes() == want_s.tobytes() and np.array_equal(un_p, win), name
        bands = [(np.zeros(ns, dtype=np.int32), npos)] + [hugging_band(win, npos, m) for m in (0, 1, 5)]
        for low, width in bands:
            assert band_contains(win, low, width), (name, width)
            got_s, got_p = np_squiggle_match_banded(low, width, sig[start:end], params, *pens, viterbi=True)
            assert np.float32(got_s).tobytes() == want_s.tobytes(), (name, width, got_s, want_s)
            assert got_p is not None and np.array_equal(got_p, win), (name, width)
            nbands += 1
        for dt in (np.float32, np.float64):
            a = np_squiggle_match_banded(bands[0][0], npos, sig[start:end], params, *pens, viterbi=False, dtype=dt)[0]
            b = np_squiggle_match(sig[start:end], params, *pens, viterbi=False, dtype=dt)[0]
            assert dt(a).tobytes() == dt(b).tobytes(), (name, dt)
    assert nbands >= 80


def test_a_band_that_misses_the_path_scores_lower():
    params, sig, _ = synth.simulated_squiggle(120, 31)
    pens = PENS[0]
    un_s, un_p = np_squiggle_match(sig, params, *pens)
    low = np.full(len(sig), 100, dtype=np.int32)             # only the squiggle's last 20 positions
    got_s, got_p = np_squiggle_match_banded(low, 20, sig, params, *pens)
    assert got_s < un_s and got_s > -1e29 and got_p is not None and np.all((got_p == -1) | (got_p >= 100))


def _diagonal_formula(ns, npos, h):
    width = min(npos, 2 * h + 1)
    return [min(max(t * npos // ns - h, 0), npos - width) for t in range(ns)], width


def test_diagonal_band_equals_its_formula():
    for ns in (1, 2, 3, 7, 64, 65, 500):
        for npos in (1, 2, 3, 5, 64, 65, 257, 1000):
            for h in (0, 1, 2, 31, 32, 128, (npos - 1) // 2, npos // 2, npos, 5000):
                low, width = sa.squiggle_diagonal_band(ns, npos, h)
                want_low, want_w = _diagonal_formula(ns, npos, h)
                assert width == want_w and low.dtype == np.int32 and low.tolist() == want_low, (ns, npos, h)
                assert np.all(np.diff(low) >= 0) and low.min() >= 0 and low.max() <= npos - width
    # 64-bit products, and the width alone
    low, width = sa.squiggle_diagonal_band(100000, 1 << 20, 3)
    assert width == 7 and low[-1] == 99999 * (1 << 20) // 100000 - 3 and np.all(np.diff(low) >= 0)
    assert sa.lib().scrappie_hip_squiggle_diagonal_band(10, 50, 2, None) == 5
    assert sa.squiggle_diagonal_band(0, 10, 2)[1] == 5 and len(sa.squiggle_diagonal_band(0, 10, 2)[0]) == 0


def test_band_argument_errors_without_gpu():
    """an invalid band: NAN and a telling text from the per-read functions, ValueError from the Python layer where it can
    tell, and nothing is launched (this runs without a GPU)"""
    L = sa.lib()
    params, sig, _ = synth.simulated_squiggle(10, 1)
    ns = len(sig)
    pens = (1.0, 0.0, 2.0, 5000.0, 5.0)
    m = oracle.NpMat(params)
    mp = C.cast(m.ptr, C.POINTER(sa._Mat))
    rt = sa._RawTable(None, ns, 0, ns, sig.ctypes.data_as(C.POINTER(C.c_float)))
    path = np.zeros(ns, dtype=np.int32)
    pp = path.ctypes.data_as(C.POINTER(C.c_int32))
    before = sa.squiggle_band_form_counts()

    def both(low, width, word):
        lowp = None if low is None else np.ascontiguousarray(low, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        s = L.squiggle_match_viterbi_banded(rt, pens[0], mp, *pens[1:], lowp, width, pp)
        assert np.isnan(s) and word in sa.last_error(), (word, s, sa.last_error())
        s = L.squiggle_match_forward_banded(rt, pens[0], mp, *pens[1:], lowp, width)
        assert np.isnan(s) and word in sa.last_error(), (word, s, sa.last_error())

    good = np.minimum(np.arange(ns) // 4, 9)
    dec = good.copy(); dec[5] = dec[4] + 1; dec[6] = dec[4]
    both(dec, 4, "decreases")
    past = good.copy(); past[-1] = 10
    both(past, 4, "past")
    neg = good.copy(); neg[0] = -1
    both(neg, 4, "negative")
    both(good, 0, "width 0")
    both(None, 3, "without low")
    assert sa.squiggle_band_form_counts() == before
    # the per-read checks still come first
    s = L.squiggle_match_viterbi_banded(rt, 0.0, mp, *pens[1:], good.astype(np.int32).ctypes.data_as(C.POINTER(C.c_int32)), 4, pp)
    assert np.isnan(s) and "rate" in sa.last_error()
    # the Python layer
    raw = sa.RawTable(sig)
    with pytest.raises(ValueError):
        sa.squiggle_match(raw, params, band=(good[:-1], 4))            # one entry per mapped sample
    with pytest.raises(ValueError):
        sa.squiggle_match(raw, params, band=(good, -1))
    with pytest.raises(ValueError):
        sa.squiggle_diagonal_band(10, 10, -1)
    with pytest.raises(RuntimeError, match="decreases"):
        sa.squiggle_match(raw, params, band=(dec, 4))


def test_band_plan_keeps_neighbours_apart():
    """scrappie_hip_squiggle_band_plan: per read nsample x 8 ceil(width / 64) code words and nsample END words (rounded to 16
    bytes); scratch rows of 2 (2 width + 1) floats for widths beyond the LDS home, none (-1) within it; every start 16-byte
    aligned, neighbours disjoint, the allocation covers the last read; a width above npos counts as npos"""
    M = int(sa.lib().scrappie_hip_squiggle_band_lds_max_width())
    assert 1000 < M < 16384 and (16 + 2 * (2 * M + 1)) * 4 <= 65536 < (16 + 2 * (2 * (M + 1) + 1)) * 4
    width = [1, M + 1, 64, M + 2, 65, M, M + 3, 257, 2 * M + 1, M + 4, 3, M + 5]
    rng = np.random.default_rng(7)
    for order in (np.arange(len(width)), np.arange(len(width))[::-1], rng.permutation(len(width)), rng.permutation(len(width))):
        W = [width[i] for i in order]
        NS = [(1, 2, 3, 64, 65, 257, 400)[i % 7] for i in range(len(W))]
        NPOS = [3 * M] * len(W)
        for path in (True, False):
            pl = sa.plan_squiggle_band(NPOS, W, NS, path=path)
            scr, tb = pl["scr_off"], pl["tb_off"]
            ends_scr, ends_tb = [], []
            for i, (w, ns) in enumerate(zip(W, NS)):
                if w <= M:
                    assert scr[i] == -1, (i, w)
                else:
                    assert scr[i] >= 0 and scr[i] % 4 == 0, (i, w)
                    ends_scr.append((int(scr[i]), int(scr[i]) + 2 * (2 * w + 1)))
                if path:
                    words = ns * 8 * ((w + 63) // 64) + ns
                    assert tb[i] >= 0 and tb[i] % 4 == 0, (i, w)
                    ends_tb.append((int(tb[i]), int(tb[i]) + words))
                else:
                    assert tb[i] == -1
            for ends, total in ((ends_scr, pl["scr_floats"]), (ends_tb, pl["tb_words"])):
                ends.sort()
                for (a0, a1), (b0, b1) in zip(ends, ends[1:]):
                    assert a1 <= b0, (ends, order)
                assert (ends[-1][1] if ends else 0) <= total
                assert total <= sum((b - a + 3) & ~3 for a, b in ends)               # and nothing beyond the rounding
            assert pl["bytes"] >= 4 * (pl["scr_floats"] + pl["tb_words"])
    # a width above npos is npos: the same plan
    a, b = sa.plan_squiggle_band([100, 5000], [100, 5000], [10, 10]), sa.plan_squiggle_band([100, 5000], [7000, 1 << 40], [10, 10])
    assert a["bytes"] == b["bytes"] and a["tb_words"] == b["tb_words"] and a["scr_floats"] == b["scr_floats"]
    # what a band saves: the profile's longest read, 81106 samples x 10138 positions
    full = 81106 * 8 * ((10138 + 63) // 64) * 4
    band = sa.plan_squiggle_band([10138], [1025], [81106])
    assert band["tb_words"] * 4 < full / 9 and band["scr_off"][0] == -1
