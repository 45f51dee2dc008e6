"""The banded forms of k_map_edits_rows and k_map_edits on the device (csrc/sh_map_edits.h): the per-read symbol
map_post_edits_banded on dense synthetic posteriors against the float32 restatement np_map_edits_band
(tests/test_map_edits_band_cpu.py) -- Viterbi in bits for base, sub, del, ins and the NaN pattern, at 64 and at 256 positions per
workgroup (the two in each other's bits); forward within the standing bound 2 |np32 - f64| + 1e-5 |f64| against the float64
restatement -- at the 64-cell groups and the 256-position chunks, few blocks and many, in the full band (map_post_edits' bits), path
bands, a diagonal band, a high edge that jumps, a low edge that waits and jumps, an empty entry and a tight band; base in a band that
holds the path against k_map's unbanded score; the batched engine against the per-read symbol on the read's own posterior in bits
under every cut; the scratch of the forms; the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_gpu_map_crf import READ, READS, _prepared
from test_map_edits_band_cpu import CASES as CPU_CASES, full_band, np_bounds_sane, np_map_edits_band
from test_map_edits_cpu import PENS, make_post

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
TR = "rgrgr_r94"
WIDTHS = (64, 256)
# (name, k, n, NB): the states at the edges of a 64-cell group, of a 256-position chunk and of two of them; one with about 2 n blocks
STATE_SHAPES = [("k2-n63", 2, 63, 70), ("k3-n64", 3, 64, 60), ("k5-n65", 5, 65, 80), ("k3-n65-two-n-blocks", 3, 65, 130),
                ("k2-n255", 2, 255, 200), ("k3-n256", 3, 256, 300), ("k5-n257", 5, 257, 260), ("k5-n513", 5, 513, 400)]
BLOCK_COUNTS = (1, 3, 4, 5, 8, 9)        # around SH_ME_CH = SH_ME_D = 4 and twice that
KINDS = ("path1", "path8", "diagonal", "high-jump", "low-waits")
# (above 100 states the restatement takes a second or two: the diagonal band runs at n = 256 alone, the narrowest path band -- where T0, T1 and the
# first 64-cell group of an entry move most -- at 256, 257 and 513, the edges of one and of two 256-position chunks)
SHAPE_KINDS = [(s, kd) for s in STATE_SHAPES for kd in KINDS
               if s[2] < 100 or s[2] == 256 or kd not in ("path1", "diagonal") or (kd == "path1" and s[2] in (257, 513))]


def _str(codes):
    return "".join("ACGT"[b] for b in codes)


def flat(res):
    return np.concatenate([np.ravel(res[1]), np.ravel(res[2]), np.ravel(res[3])]).astype(np.float64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def same_results(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def worst():
    return dict(ratio=0.0, checked=0)


@pytest.fixture(scope="module", autouse=True)
def default_width_afterwards():
    yield
    sa.lib().scrappie_hip_debug_option(None, b"map_edits_band_width", 0)


def at_width(w, fn):
    """fn() with the banded k_map_edits at w positions per workgroup (0: the default) on the per-read surface's engine"""
    assert sa.lib().scrappie_hip_debug_option(None, b"map_edits_band_width", w) == 0, sa.last_error()
    try:
        return fn()
    finally:
        sa.lib().scrappie_hip_debug_option(None, b"map_edits_band_width", 0)


def shape_case(k, n, NB):
    rng = np.random.default_rng(900 + 17 * n + NB + k)
    return make_post(NB, k, rng), rng.integers(0, 4, n + k - 1).astype(np.int32), PENS[(n + NB) % 2]


def diagonal(NB, n, h):
    lo, hi = sa.diagonal_bands(h, NB, n)
    lo[0], hi[-1] = 0, n
    return lo, hi


def band_of_kind(kind, m, seq, k, pens, NB):
    """(low, high) of a kind for a case, around k_map's own unbanded Viterbi path where the kind needs one"""
    n = len(seq) - k + 1
    if kind == "full":
        return full_band(NB, n)
    if kind == "diagonal":
        return diagonal(NB, n, 3)
    path = sa.map_post_to_sequence(m, _str(seq), *pens, viterbi=True, path=True)[1]
    if kind == "path1":
        return sa.map_path_band(path, n, 1)
    lo, hi = (x.astype(np.int64) for x in sa.map_path_band(path, n, 8))
    if kind == "high-jump":                                 # high goes to n in one block, from more than 256 states (where there are as many) below it
        t0 = max(int(np.searchsorted(hi, max(n - 300, n // 3))), 1)
        hi[t0:] = n
    elif kind == "low-waits":                               # low stays at 0 over the first half of the blocks, then jumps to the path's
        lo[:NB // 2] = 0
    elif kind == "empty-entry":
        t = NB // 2
        lo[t] = hi[t] = hi[t - 1]
        lo = np.maximum.accumulate(lo)
        hi = np.maximum(hi, lo)
    else:
        assert kind == "path8", kind
    assert np_bounds_sane(lo, hi, NB, n), kind
    return lo.astype(np.uintp), hi.astype(np.uintp)


def check_band(post, seq, k, pens, lo, hi, worst, tag, holds_path=False):
    """both widths, Viterbi in bits against the float32 restatement and each other, forward within the standing bound"""
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    codes = np.asarray(seq, dtype=np.int32)
    want = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=True)
    got = {w: at_width(w, lambda: sa.map_post_edits(m, codes, *pens, viterbi=True, bands=(lo, hi))) for w in WIDTHS}
    for w in WIDTHS:
        for name, g, x in zip(("base", "sub", "del", "ins"), got[w], want):
            assert same_bits(g, x), (tag, w, name, np.flatnonzero(np.ravel(np.asarray(g, dtype=np.float32)).view(np.int32) != np.ravel(np.asarray(x, dtype=np.float32)).view(np.int32))[:8])
    assert same_results(got[64], got[256]), tag
    if holds_path:                                          # base: k_map's unbanded score of the sequence itself
        assert same_bits(got[64][0], sa.map_post_to_sequence(m, _str(seq), *pens, viterbi=True)[0]), tag
    f32r = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=False)
    f32 = flat(f32r)
    f64r = np_map_edits_band(post, seq, k, pens, lo, hi, viterbi=False, dtype=np.float64)
    f64 = flat(f64r)
    ok = ~np.isnan(f64)
    bound = 2 * np.abs(f32[ok] - f64[ok]) + 1e-5 * np.abs(f64[ok])
    for w in WIDTHS:
        fw = at_width(w, lambda: sa.map_post_edits(m, codes, *pens, viterbi=False, bands=(lo, hi)))
        g = flat(fw)
        assert np.array_equal(np.isnan(g), np.isnan(f64)), (tag, w, np.flatnonzero(np.isnan(g) != np.isnan(f64))[:8])
        err = np.abs(g[ok] - f64[ok])
        ratio = float(np.max(err / (bound + 1e-30))) if err.size else 0.0
        print("%s, %d positions per workgroup: forward worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f over %d scores" % (tag, w, ratio, err.size))
        assert np.all(err <= bound), (tag, w, float(np.max(err - bound)))
        b64 = float(f64r[0])                                # base: the same bound (below -1e30 / 2 there is no path: -1e30 as it is)
        assert abs(float(fw[0]) - b64) <= 2 * abs(float(f32r[0]) - b64) + 1e-5 * abs(b64), (tag, w, fw[0], b64)
        worst["ratio"] = max(worst["ratio"], ratio)
        worst["checked"] += int(err.size)


# ---------------------------------------------------------------------------
# the per-read symbol
# ---------------------------------------------------------------------------
def test_the_smallest_case_first(worst):
    """k = 2, three bases, two states, three blocks, the full band: the first launch of the banded kernels"""
    rng = np.random.default_rng(1)
    post, seq = make_post(3, 2, rng), rng.integers(0, 4, 3)
    check_band(post, seq, 2, PENS[0], *full_band(3, 2), worst, "smallest")


@pytest.mark.parametrize("case", [c for c in CPU_CASES if c[7] == "special" or c[0].startswith(("k1-L12", "k2-L14", "k3-L20-nb45"))], ids=lambda c: c[0])
def test_cpu_cases_on_the_device(case, worst):
    """the special bands of the CPU test -- an empty entry, low[NB - 1] == n, START in block 0 only, the tight band with NaN ends -- and
    some of its path and diagonal bands"""
    name, post, seq, k, pens, lo, hi, kind = case
    check_band(post, seq, k, pens, lo, hi, worst, name, holds_path=kind == "path")
    if name == "tight-ends":
        m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
        base, sub, dele, ins = sa.map_post_edits(m, seq, *pens, viterbi=True, bands=(lo, hi))
        assert np.isfinite(base) and np.any(np.isnan(ins[0])) and np.all(np.isfinite(sub[4]))


@pytest.mark.parametrize("NB", BLOCK_COUNTS)
def test_block_counts(NB, worst):
    """k = 2, seven states: the staging and load-ahead depths, in the full band and the widest diagonal one the block count allows"""
    post, seq, pens = shape_case(2, 7, NB)
    check_band(post, seq, 2, pens, *full_band(NB, 7), worst, "nb%d-full" % NB)
    if NB >= 4:
        lo, hi = diagonal(NB, 7, 2)
        assert np_bounds_sane(lo, hi, NB, 7)
        check_band(post, seq, 2, pens, lo, hi, worst, "nb%d-diagonal" % NB)


@pytest.mark.parametrize("shape", STATE_SHAPES, ids=[s[0] for s in STATE_SHAPES])
def test_full_band_has_the_bits_of_the_unbanded_call(shape):
    """every output, both forms, both widths: map_post_edits' bits"""
    name, k, n, NB = shape
    post, seq, pens = shape_case(k, n, NB)
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    lo, hi = full_band(NB, n)
    for vit in (True, False):
        want = sa.map_post_edits(m, seq, *pens, viterbi=vit)
        assert np.any(np.isfinite(want[1]))
        for w in WIDTHS:
            got = at_width(w, lambda: sa.map_post_edits(m, seq, *pens, viterbi=vit, bands=(lo, hi)))
            assert same_results(got, want), (name, vit, w)


@pytest.mark.parametrize("shape,kind", SHAPE_KINDS, ids=["%s-%s" % (s[0], kd) for s, kd in SHAPE_KINDS])
def test_shapes_against_restatement(shape, kind, worst):
    name, k, n, NB = shape
    post, seq, pens = shape_case(k, n, NB)
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    lo, hi = band_of_kind(kind, m, seq, k, pens, NB)
    if kind == "high-jump" and n > 300:
        assert np.max(np.diff(np.asarray(hi, dtype=np.int64))) > 256
    check_band(post, seq, k, pens, lo, hi, worst, "%s-%s" % (name, kind), holds_path=kind != "diagonal")


def test_an_empty_entry_in_a_long_read(worst):
    post, seq, pens = shape_case(3, 65, 130)
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    lo, hi = band_of_kind("empty-entry", m, seq, 3, pens, 130)
    assert np.any(lo == hi)
    check_band(post, seq, 3, pens, lo, hi, worst, "k3-n65-empty-entry")


def test_bad_bands_per_read():
    rng = np.random.default_rng(2)
    post = make_post(30, 3, rng)
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    seq = rng.integers(0, 4, 14).astype(np.int32)
    lo, hi = full_band(30, 12)
    with pytest.raises(ValueError):
        sa.map_post_edits(m, seq, bands=(lo, hi - 1))       # does not end at n
    fp, sp, ip = C.POINTER(C.c_float), C.POINTER(C.c_size_t), C.POINTER(C.c_int)
    bad = (hi - 1).astype(np.uintp)
    base = C.c_float(0.0)
    sub = np.zeros(4 * 14, dtype=np.float32)
    rc = sa.lib().map_post_edits_banded(m.data(), 0.0, 0.0, 4.0, seq.ctypes.data_as(ip), 14, lo.ctypes.data_as(sp), bad.ctypes.data_as(sp), 1, C.byref(base),
                                        sub.ctypes.data_as(fp), None, None)
    assert rc == 0 and np.isnan(base.value) and np.all(np.isnan(sub)) and "bands are not valid" in sa.last_error(), sa.last_error()
    for s, text in (([0, 4, 1, 2], "not a base"), ([0, 1], "shorter than the model's k-mer")):
        s = np.asarray(s, dtype=np.int32)
        rc = sa.lib().map_post_edits_banded(m.data(), 0.0, 0.0, 4.0, s.ctypes.data_as(ip), len(s), lo.ctypes.data_as(sp), hi.ctypes.data_as(sp), 1, C.byref(base), None, None, None)
        assert rc == 0 and np.isnan(base.value) and text in sa.last_error(), sa.last_error()
    assert sa.lib().scrappie_hip_debug_option(None, b"map_edits_band_width", 128) != 0 and "64 or 256" in sa.last_error()


def test_no_banded_form_needs_scratch():
    sc = sa.map_edits_band_scratch()
    print("scratch bytes per lane by banded form: %r" % sorted(sc.items()))
    assert len(sc) == 16 and all(v == 0 for v in sc.values()), sc


# ---------------------------------------------------------------------------
# the batched engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    e.load_model(TR, model.synthetic_model(TR, seed=1))
    yield e
    e.close()


def _sig(n, seed):
    return synth.medmad_normalise(synth.synthetic_signal(n, seed))


@pytest.fixture(scope="module")
def call(eng):
    """four reads of 400 .. 1000 samples, a draft of a third of its blocks in bases each, the bands of half-width 8 around their paths
    and the per-read symbol's results on eng.posterior, banded and not"""
    rng = np.random.default_rng(47)
    sigs = [_sig(n, 300 + i) for i, n in enumerate((400, 1000, 640, 815))]
    posts = [eng.posterior(x, TR) for x in sigs]
    seqs = [rng.integers(0, 4, len(p) // 3).astype(np.int32) for p in posts]
    mapped = eng.map_to_sequence(sigs, [_str(s) for s in seqs], viterbi=True, path=True)
    bands = [sa.map_path_band(pth, len(s) - 4, 8) for (sc, pth), s in zip(mapped, seqs)]
    mats = [sa.ScrappyMatrix.from_numpy(p, sloika=False) for p in posts]
    banded = {vit: [sa.map_post_edits(m, s, viterbi=vit, bands=b) for m, s, b in zip(mats, seqs, bands)] for vit in (True, False)}
    plain = {vit: [sa.map_post_edits(m, s, viterbi=vit) for m, s in zip(mats, seqs)] for vit in (True, False)}
    return dict(sigs=sigs, posts=posts, seqs=seqs, bands=bands, mats=mats, banded=banded, plain=plain, scores=[sc for sc, pth in mapped])


@pytest.mark.parametrize("viterbi", [True, False])
def test_engine_in_bits_under_every_cut(eng, call, viterbi):
    """the per-read symbol on eng.posterior, in bits, in one launch and under budgets that cut after every read and after every second;
    fewer launches in the band than without one at the same budget"""
    key = ("edits", viterbi, True, 64)
    rows = [sa.map_edits_band_row_bytes(*b) for b in call["bands"]]
    launches = {}
    for kb in (0, 1, (max(rows) + min(rows)) // 1024 + 64):
        eng.debug_option("map_edits_budget_kb", kb)
        try:
            before = sum(v for q, v in sa.map_edits_band_form_counts().items() if q[0] == "edits")
            res = eng.score_edits_transducer(call["sigs"], call["seqs"], viterbi=viterbi, bands=call["bands"])
            launches[kb] = sum(v for q, v in sa.map_edits_band_form_counts().items() if q[0] == "edits") - before
            assert eng.map_edits_timing()["launches"] == launches[kb]
            if kb:
                plain = eng.score_edits_transducer(call["sigs"], call["seqs"], viterbi=viterbi)
                unbanded = eng.map_edits_timing()["launches"]
        finally:
            eng.debug_option("map_edits_budget_kb", 0)
        for i, (r, w) in enumerate(zip(res, call["banded"][viterbi])):
            assert same_results(r, w), (kb, i)
            assert np.isfinite(r[0]) and np.any(np.isfinite(r[1])), i
        if kb > 1:
            print("budget %d KB: %d launches in the band, %d without" % (kb, launches[kb], unbanded))
            assert launches[kb] < unbanded
            for i, (r, w) in enumerate(zip(plain, call["plain"][viterbi])):
                assert same_results(r, w), i
    assert launches[0] == 1 and launches[1] == len(call["sigs"]) and 1 < launches[max(launches)] < len(call["sigs"]), launches
    assert eng.map_edits_timing()["row_bytes"] > 0
    if viterbi:                                             # the bands hold the paths: base is k_map's unbanded score through the mapping engine
        for r, sc in zip(res, call["scores"]):
            assert same_bits(r[0], sc)
    assert key in sa.map_edits_band_form_counts()


def test_engine_widths_agree_and_are_counted(eng, call):
    got = {}
    for w in WIDTHS:
        before = sa.map_edits_band_form_counts()
        eng.debug_option("map_edits_band_width", w)
        try:
            got[w] = eng.score_edits_transducer(call["sigs"], call["seqs"], viterbi=True, bands=call["bands"])
        finally:
            eng.debug_option("map_edits_band_width", 0)
        now = sa.map_edits_band_form_counts()
        assert now["edits", True, True, w] == before["edits", True, True, w] + 1
        assert now["edits", True, True, 320 - w] == before["edits", True, True, 320 - w]
    for a, b in zip(got[64], got[256]):
        assert same_results(a, b)


def test_engine_bad_band_and_no_band_beside_good_ones(eng, call):
    """read 1 with a band made for another block count: NaN, its neighbours scored; read 2 without a band: the unbanded forms, counted"""
    bands = list(call["bands"])
    bands[1] = (bands[1][0][:-1], bands[1][1][:-1])
    bands[2] = None
    ub, bb = sa.map_edits_form_counts(), sa.map_edits_band_form_counts()
    res = eng.score_edits_transducer(call["sigs"], call["seqs"], viterbi=True, bands=bands)
    assert "read 1" in sa.last_error() and "bands are not valid" in sa.last_error(), sa.last_error()
    ua, ba = sa.map_edits_form_counts(), sa.map_edits_band_form_counts()
    assert np.isnan(res[1][0]) and all(np.all(np.isnan(a)) for a in res[1][1:])
    assert same_results(res[0], call["banded"][True][0]) and same_results(res[3], call["banded"][True][3])
    assert same_results(res[2], call["plain"][True][2])
    assert ua["edits", True, True] == ub["edits", True, True] + 1 and ua["rows", True, True, False] == ub["rows", True, True, False] + 1
    assert sum(v for q, v in ba.items() if q[0] == "edits") == sum(v for q, v in bb.items() if q[0] == "edits") + 1
    # an int: scrappy's diagonal band per read; one pair for all reads is refused for the reads it does not fit
    res = eng.score_edits_transducer(call["sigs"][:2], call["seqs"][:2], viterbi=False, bands=40)
    assert all(np.isfinite(r[0]) for r in res)


def test_crf_model_is_refused(eng, call):
    eng.load_model("rnnrf_r94", model.synthetic_model("rnnrf_r94", seed=11))
    with pytest.raises(RuntimeError, match="rnnrf_r94.*flip-flop"):
        eng.score_edits_transducer(call["sigs"][:2], "ACGTACGTAC", model="rnnrf_r94", bands=8)
    assert "scrappie_hip_map_crf_edits_banded_batch" in sa.last_error()


def test_seqmappy_kmer_edits_band_cli(eng, tmp_path):
    """`scrappie seqmappy --kmer-edits --band 8` on the bundled read: Engine.score_edits_transducer(..., bands=...)'s table in the band
    around the path of Engine.map_to_sequence"""
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    nblock = eng.read_blocks(TR, len(x))
    seq = np.random.default_rng(5).integers(0, 4, nblock // 3).astype(np.int32)
    fa = str(tmp_path / "draft.fa")
    with open(fa, "w") as fh:
        fh.write(">draft\n%s\n" % _str(seq))
    tr_file = str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(model.synthetic_model(TR, seed=1), tr_file)
    ((score, path),) = eng.map_to_sequence([x], [_str(seq)], viterbi=True, path=True)
    band = sa.map_path_band(path, len(seq) - 4, 8)
    ((base, sub, dele, ins),) = eng.score_edits_transducer([x], [seq], viterbi=True, bands=[band])
    L = len(seq)

    def f(v):
        d = np.float32(v) - np.float32(base)
        return "nan" if np.isnan(d) else "%f" % d
    want = "# %s to %s -- edits of %d bases, score %f over %d blocks\n" % (f5, fa, L, base, nblock)
    want += "pos\tbase\tdel\tsubA\tsubC\tsubG\tsubT\tinsA\tinsC\tinsG\tinsT\n"
    for i in range(L):
        want += "\t".join(["%d" % i, "ACGT"[seq[i]], f(dele[i])] + [f(v) for v in sub[i]] + [f(v) for v in ins[i]]) + "\n"
    want += "\t".join(["%d" % L] + ["-"] * 6 + [f(v) for v in ins[L]]) + "\n"
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--kmer-edits", "--band", "8", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--kmer-edits", "--band", "0", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout == "" and "at least 1" in r.stderr


def test_summary(worst):
    print("forward: worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f over %d scores in bands" % (worst["ratio"], worst["checked"]))
    assert worst["checked"] > 10000
