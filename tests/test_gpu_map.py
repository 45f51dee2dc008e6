"""Block-based mapping on the GPU (sh_map.h): the per-read map_to_sequence_* against the reference's compiled
decode.c (oracle/_ref/libref_decode.so) and the numpy restatement of tests/test_map_cpu.py; the batched
Engine.map_to_sequence against the reference run on the engine's own posterior; `scrappie seqmappy` on the bundled
reads.  Viterbi scores and paths must be bit-identical; forward within 2x the reference's own error + 1e-5 |score|."""
import ctypes as C
import hashlib
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_map_cpu import band_sets, call_map, lds_max_seq, map_cases, map_form, map_scratch_cases, np_map, ref_decode_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
READS = os.path.join(ROOT, "tests", "golden", "reads")
FA_SHA256 = {
    "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand":
        "0dcf90a5b480a0765f5090e4c888a946330a956aad9cc2596f53e474ad0a2786",
    "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch271_read66_strand":
        "e56d9dc82d910b61ed30656ebb6035fefc029da2a675025eaa0f90b7a7e7e6b4",
}
PM = C.POINTER(sa._Mat)


@pytest.fixture(scope="module")
def ref():
    R = ref_decode_lib()
    assert R is not None, "oracle/_ref/libref_decode.so is required (build() makes it and it travels with the tree)"
    return R


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """k_map launches per form before this module's first test (test_every_map_form_was_launched)"""
    return sa.launch_form_counts()["map"]


def _f64(post, seq, pens, bands=None):
    lo, hi = (None, None) if bands is None else bands
    return float(np_map(post, seq, *pens, viterbi=False, low=lo, high=hi, dtype=np.float64)[0])


def _forward_ok(got, want_ref, post, seq, pens, bands=None, exact=None):
    """|gpu - f64| <= 2 |ref - f64| + 1e-5 |score|; returns the ratio |gpu - f64| / (|ref - f64| + 1e-5 |score|)"""
    if exact is None:
        exact = _f64(post, seq, pens, bands)
    eg, er = abs(float(got) - exact), abs(float(want_ref) - exact)
    assert eg <= 2 * er + 1e-5 * abs(exact), (got, want_ref, exact)
    return eg / (er + 1e-5 * abs(exact) + 1e-30)


def test_per_read_against_reference(ref):
    L = sa.lib()
    rng = np.random.default_rng(21)
    worst = 0.0
    n_band = 0
    for name, post, seq, pens in map_cases():
        want_s, want_p = call_map(ref, post, seq, pens, True)
        got_s, got_p = call_map(L, post, seq, pens, True, cast=PM)
        assert got_s.tobytes() == want_s.tobytes(), (name, got_s, want_s)
        assert np.array_equal(got_p, want_p), name
        np_s, np_p = np_map(post, seq, *pens)
        assert np.float32(np_s).tobytes() == got_s.tobytes() and np.array_equal(np_p, got_p), name
        want_f, _ = call_map(ref, post, seq, pens, False)
        got_f, _ = call_map(L, post, seq, pens, False, cast=PM)
        worst = max(worst, _forward_ok(got_f, want_f, post, seq, pens))
        if len(seq) < 3 or post.shape[0] > 2000:
            continue
        for bname, bands in band_sets(post.shape[0], len(seq), rng):
            lo, hi = bands
            if not ref.are_bounds_sane(lo.ctypes.data_as(C.POINTER(C.c_size_t)), hi.ctypes.data_as(C.POINTER(C.c_size_t)),
                                       post.shape[0], len(seq)):
                got_s, _ = call_map(L, post, seq, pens, True, bands, cast=PM)
                assert np.isnan(got_s), (name, bname)
                continue
            n_band += 1
            want_s, _ = call_map(ref, post, seq, pens, True, bands)
            got_s, _ = call_map(L, post, seq, pens, True, bands, cast=PM)
            assert got_s.tobytes() == want_s.tobytes(), (name, bname, got_s, want_s)
            want_f, _ = call_map(ref, post, seq, pens, False, bands)
            got_f, _ = call_map(L, post, seq, pens, False, bands, cast=PM)
            worst = max(worst, _forward_ok(got_f, want_f, post, seq, pens, bands))
    assert n_band > 100
    print("forward: worst |gpu - f64| / (|ref - f64| + 1e-5 |score|) = %.3f" % worst)


def _sane_ref(ref, bands, nblock, L):
    sp = C.POINTER(C.c_size_t)
    return bool(ref.are_bounds_sane(bands[0].ctypes.data_as(sp), bands[1].ctypes.data_as(sp), nblock, L))


@pytest.fixture(scope="module")
def scratch_cases(ref):
    """map_scratch_cases with what the reference and the restatement give for each, computed once: unbanded
    (ref_v, ref_f, np_v, f64); per band set (name, bands, sane, ref_v, ref_f, f64)"""
    out = []
    for name, post, seq, pens, bsets in map_scratch_cases():
        c = dict(name=name, post=post, seq=seq, pens=pens, bands=None)
        if bsets is None:
            c["ref_v"] = call_map(ref, post, seq, pens, True)
            c["ref_f"] = call_map(ref, post, seq, pens, False)[0]
            c["np_v"] = np_map(post, seq, *pens)
            c["f64"] = _f64(post, seq, pens)
        else:
            c["bands"] = []
            for bname, bands in bsets:
                b = dict(name=bname, bands=bands, sane=_sane_ref(ref, bands, post.shape[0], len(seq)))
                if b["sane"]:
                    b["ref_v"] = call_map(ref, post, seq, pens, True, bands)[0]
                    b["ref_f"] = call_map(ref, post, seq, pens, False, bands)[0]
                    b["f64"] = _f64(post, seq, pens, bands)
                c["bands"].append(b)
        out.append(c)
    return out


def test_per_read_scratch_cases(scratch_cases):
    """the scratch home (and its control at the last LDS length) through the per-read surface: unbanded Viterbi score and
    path byte for byte against the reference and the restatement, banded Viterbi against the reference, forward by
    _forward_ok, NaN where are_bounds_sane refuses"""
    L = sa.lib()
    M = lds_max_seq()
    worst = {False: 0.0, True: 0.0}                      # by home: scratch?
    n_band = 0
    ran = set()
    before = sa.launch_form_counts()["map"]
    for c in scratch_cases:
        name, post, seq, pens = c["name"], c["post"], c["seq"], c["pens"]
        scr = len(seq) > M
        if c["bands"] is None:
            want_s, want_p = c["ref_v"]
            got_s, got_p = call_map(L, post, seq, pens, True, cast=PM)
            assert got_s.tobytes() == want_s.tobytes(), (name, got_s, want_s)
            assert np.array_equal(got_p, want_p), name
            np_s, np_p = c["np_v"]
            assert np.float32(np_s).tobytes() == got_s.tobytes() and np.array_equal(np_p, got_p), name
            got_f, _ = call_map(L, post, seq, pens, False, cast=PM)
            worst[scr] = max(worst[scr], _forward_ok(got_f, c["ref_f"], post, seq, pens, exact=c["f64"]))
            ran |= {map_form(post, seq, None, v, M=M) for v in (True, False)}
            continue
        for b in c["bands"]:
            bands = b["bands"]
            got_s, _ = call_map(L, post, seq, pens, True, bands, cast=PM)
            if not b["sane"]:
                assert np.isnan(got_s), (name, b["name"])
                continue
            n_band += scr
            assert got_s.tobytes() == b["ref_v"].tobytes(), (name, b["name"], got_s, b["ref_v"])
            got_f, _ = call_map(L, post, seq, pens, False, bands, cast=PM)
            worst[scr] = max(worst[scr], _forward_ok(got_f, b["ref_f"], post, seq, pens, bands, exact=b["f64"]))
            ran |= {map_form(post, seq, bands, v, M=M) for v in (True, False)}
    after = sa.launch_form_counts()["map"]
    assert n_band >= 12
    assert ran == {(v, b, False, h) for v in (True, False) for b in (True, False) for h in (True, False)}
    for k in after:
        assert (after[k] > before[k]) == (k in ran), (k, before[k], after[k])       # the forms the shapes imply are the forms launched
    print("sane banded scratch cases: %d" % n_band)
    print("forward: worst |gpu - f64| / (|ref - f64| + 1e-5 |score|) = %.3f in LDS (the control), %.3f in scratch" % (worst[False], worst[True]))


def test_undefined_cases_give_nan():
    L = sa.lib()
    post, _ = synth.simulated_posterior(50, 3, klen=3)
    seq = np.arange(10, dtype=np.int32)
    assert np.isnan(call_map(L, post, seq[:0], (0.0, 0.0, 4.0), True, cast=PM)[0])
    assert "empty" in sa.last_error()
    bad = seq.copy(); bad[4] = 64                                      # nr - 1 = 64 k-mers
    assert np.isnan(call_map(L, post, bad, (0.0, 0.0, 4.0), False, cast=PM)[0])
    short = seq[:2]
    bands = (np.zeros(50, dtype=np.uintp), np.full(50, 2, dtype=np.uintp))
    assert np.isnan(call_map(L, post, short, (0.0, 0.0, 4.0), True, bands, cast=PM)[0])
    bands = (np.ones(50, dtype=np.uintp), np.full(50, 10, dtype=np.uintp))   # low[0] != 0
    assert np.isnan(call_map(L, post, seq, (0.0, 0.0, 4.0), True, bands, cast=PM)[0])


def test_true_sequence_outscores_random():
    post, tpath = synth.simulated_posterior(800, 8, klen=5)
    true = np.array([x for x in tpath if x >= 0], dtype=np.int32)
    rnd = np.random.default_rng(2).integers(0, 1024, len(true)).astype(np.int32)
    L = sa.lib()
    for vit in (True, False):
        assert call_map(L, post, true, (0.0, 0.0, 4.0), vit, cast=PM)[0] > call_map(L, post, rnd, (0.0, 0.0, 4.0), vit, cast=PM)[0]


def test_scrappy_style_map_post_to_sequence(ref):
    post, tpath = synth.simulated_posterior(300, 4, klen=4)
    bases = "".join(np.random.default_rng(4).choice(list("ACGT"), 200))
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    codes = sa.encode_bases(bases, 4)
    s, p = sa.map_post_to_sequence(m, bases, viterbi=True, path=True)
    ws, wp = call_map(ref, post, codes, (0.0, 0.0, 4.0), True)
    assert np.float32(s).tobytes() == ws.tobytes() and np.array_equal(p, wp)
    s, p = sa.map_post_to_sequence(m, bases, viterbi=True, bands=5)
    ws, _ = call_map(ref, post, codes, (0.0, 0.0, 4.0), True, sa.diagonal_bands(5, 300, len(codes)))
    assert p is None and np.float32(s).tobytes() == ws.tobytes()


@pytest.fixture(scope="module")
def eng():
    w = model.synthetic_model("rgrgr_r94", seed=1)
    e = sa.Engine(0)
    e.load_model("rgrgr_r94", w)
    yield e
    e.close()


def _bases(n, rng):
    return "".join(rng.choice(list("ACGT"), n))


def test_engine_map_to_sequence(eng, ref):
    rng = np.random.default_rng(31)
    lens = [int(x) for x in rng.integers(600, 6000, 40)]
    lens[3] = 5                                            # below the model's minimum
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 200 + i)) for i, n in enumerate(lens)]
    seqs = [_bases(int(rng.integers(8, 700)), rng) for _ in lens]
    seqs[7] = seqs[7][:20] + "N" + seqs[7][21:]          # a bad sequence
    eng.set_max_launch_reads(16)                           # >= 3 launch groups
    try:
        for vit in (True, False):
            for bands in (None, 4):
                res = eng.map_to_sequence(sigs, seqs, viterbi=vit, path=vit and bands is None, bands=bands, stay_pen=0.5,
                                          skip_pen=1.0, local_pen=4.0, min_prob=1e-5)
                assert len(res) == len(sigs)
                for i, (x, sq) in enumerate(zip(sigs, seqs)):
                    sc, pth = res[i]
                    if i in (3, 7):
                        assert np.isnan(sc) and pth is None, i
                        continue
                    post = eng.posterior(x, min_prob=1e-5)
                    codes = sa.encode_bases(sq, 5)
                    bb = None if bands is None else sa.diagonal_bands(bands, post.shape[0], len(codes))
                    if bb is not None and not ref.are_bounds_sane(bb[0].ctypes.data_as(C.POINTER(C.c_size_t)),
                                                                  bb[1].ctypes.data_as(C.POINTER(C.c_size_t)), post.shape[0], len(codes)):
                        assert np.isnan(sc), i
                        continue
                    ws, wp = call_map(ref, post, codes, (0.5, 1.0, 4.0), vit, bb)
                    if vit:
                        assert np.float32(sc).tobytes() == ws.tobytes(), (i, sc, ws)
                        if bands is None:
                            assert np.array_equal(pth, wp), i
                    else:
                        _forward_ok(sc, ws, post, codes, (0.5, 1.0, 4.0), bb)
    finally:
        eng.set_max_launch_reads(16384)


def test_engine_tiled_scratch_forms(eng, ref):
    """Engine.map_to_sequence on reads whose sequences are longer than the LDS home takes -- k_map on the tiled posterior
    with its rows in device scratch -- mixed with short ones in one call of two launch groups; one sequence of exactly M
    states (the last LDS length) and one of M + 1.  Three more scratch reads have signals of 121 to 140 blocks only: their
    sequences cannot be reached, so their scores are what START and END hold at the last block, the floats at the very
    end of a read's scratch rows, next to the first positions of the neighbouring read's rows in the same allocation.
    The reference runs on the engine's own posterior."""
    M = lds_max_seq()
    rng = np.random.default_rng(41)
    nstate = [M, M + 1, M + 600, M + 2]
    lens = [int(x) for x in rng.integers(600, 3000, 20)]
    long_at = [0, 2, 5, 17]                                # launch groups of 16 reads: two scratch reads side by side in the first, one in the second
    for i, n in zip(long_at, (28000, 28500, 29000, 28200)):
        lens[i] = n
    brief_at = [8, 9, 10]                                  # scratch reads of few blocks, neighbours in the first group
    for i, n in zip(brief_at, (605, 700, 655)):
        lens[i] = n
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 300 + i)) for i, n in enumerate(lens)]
    seqs = [_bases(int(rng.integers(8, 300)), rng) for _ in lens]
    for i, ns in zip(long_at, nstate):
        seqs[i] = _bases(ns + 4, rng)                      # k = 5: n - 4 states
    for i, ns in zip(brief_at, (M + 1, M + 4, M + 3)):     # odd and even: the rows' rounding to 16 bytes differs
        seqs[i] = _bases(ns + 4, rng)
    codes = [sa.encode_bases(sq, 5) for sq in seqs]
    assert [len(codes[i]) for i in long_at] == nstate
    posts = [eng.posterior(x, min_prob=1e-5) for x in sigs]
    assert all(5600 <= posts[i].shape[0] <= 6000 for i in long_at)
    assert [posts[i].shape[0] for i in brief_at] == [121, 140, 131]
    # (the engine cuts a call into launch groups of consecutive reads, max_launch_reads at a time while memory allows:
    # read i is in group i // 16.  The launch counts asserted at the end depend on that policy.)
    scratch_groups = {i // 16 for i, c in enumerate(codes) if len(c) > M}
    assert len(scratch_groups) == 2
    pens = (0.5, 1.0, 4.0)
    eng.set_max_launch_reads(16)                           # two launch groups, a scratch read in each
    before = sa.launch_form_counts()["map"]
    worst = {False: 0.0, True: 0.0}
    try:
        for bands in (None, 4):
            bbs = [None if bands is None else sa.diagonal_bands(bands, p.shape[0], len(c)) for p, c in zip(posts, codes)]
            sane = [bb is None or _sane_ref(ref, bb, p.shape[0], len(c)) for bb, p, c in zip(bbs, posts, codes)]
            if bands is not None:
                assert sum(sane[i] for i in long_at if len(codes[i]) > M) >= 2
            exact = [_f64(p, c, pens, bb) if ok else None for p, c, bb, ok in zip(posts, codes, bbs, sane)]
            for vit in (True, False):
                res = eng.map_to_sequence(sigs, seqs, viterbi=vit, path=vit and bands is None, bands=bands, stay_pen=pens[0],
                                          skip_pen=pens[1], local_pen=pens[2], min_prob=1e-5)
                assert len(res) == len(sigs)
                for i, (sc, pth) in enumerate(res):
                    if not sane[i]:
                        assert np.isnan(sc), i
                        continue
                    ws, wp = call_map(ref, posts[i], codes[i], pens, vit, bbs[i])
                    if vit:
                        assert np.float32(sc).tobytes() == ws.tobytes(), (i, bands, sc, ws)
                        if bands is None:
                            assert np.array_equal(pth, wp), i
                    else:
                        scr = len(codes[i]) > M
                        worst[scr] = max(worst[scr], _forward_ok(sc, ws, posts[i], codes[i], pens, bbs[i], exact=exact[i]))
    finally:
        eng.set_max_launch_reads(16384)
    after = sa.launch_form_counts()["map"]
    for v in (True, False):
        for b in (True, False):
            for h in (True, False):
                assert after[(v, b, True, h)] - before[(v, b, True, h)] >= 1, (v, b, h)
            assert after[(v, b, True, True)] - before[(v, b, True, True)] == len(scratch_groups), (v, b)      # one scratch launch per group that holds such reads
    print("forward, tiled: worst |gpu - f64| / (|ref - f64| + 1e-5 |score|) = %.3f in LDS, %.3f in scratch" % (worst[False], worst[True]))


def _fasta(name):
    path = os.path.join(READS, name + ".fa")
    data = open(path, "rb").read()
    assert hashlib.sha256(data).hexdigest() == FA_SHA256[name]
    return "".join(l.strip() for l in data.decode().splitlines()[1:])


def _prepared(path):
    L = sa.lib()
    L.scrappie_hip_read_raw.restype = sa._RawTable
    L.scrappie_hip_read_raw.argtypes = [C.c_char_p, C.c_bool]
    rt = L.scrappie_hip_read_raw(os.fsencode(path), True)
    rt = L.trim_and_segment_raw(rt, 200, 10, 100, 0.0)
    x = np.ctypeslib.as_array(rt.raw, shape=(rt.n,))[rt.start:rt.end].copy()
    sa._libc.free(C.cast(rt.raw, C.c_void_p))
    L.medmad_normalise_array(x.ctypes.data_as(C.POINTER(C.c_float)), len(x))
    return x


def test_seqmappy_bundled_reads(eng, ref, tmp_path):
    w = model.synthetic_model("rgrgr_r94", seed=1)
    mfile = str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(w, mfile)
    want = {}
    for name in FA_SHA256:
        fa, f5 = os.path.join(READS, name + ".fa"), os.path.join(READS, name + ".i16")
        codes = sa.encode_bases(_fasta(name), 5)
        post = eng.posterior(_prepared(f5), min_prob=1e-5)
        s, path = call_map(ref, post, codes, (0.0, 0.0, 4.0), True)
        nb = post.shape[0]
        per = np.float32(-s) / np.float32(nb)
        txt = "# %s to %s -- score %f over %d blocks (%f per block)\nblock\tpos\n" % (f5, fa, -s, nb, per)
        txt += "".join("%d\t%d\n" % (i, p) for i, p in enumerate(path))
        want[name] = (fa, f5, txt)
    names = list(FA_SHA256)
    one = subprocess.run([CLI, "seqmappy", "--model-file", mfile, want[names[0]][0], want[names[0]][1]],
                         capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr
    assert one.stdout == want[names[0]][2]
    two = subprocess.run([CLI, "seqmappy", "--model-file", mfile, want[names[1]][0], want[names[1]][1], want[names[0]][0], want[names[0]][1]],
                         capture_output=True, text=True, timeout=600)
    assert two.returncode == 0, two.stderr
    assert two.stdout == want[names[1]][2] + want[names[0]][2]


def test_cli_segmentation_chunk_zero_is_the_fixed_trims(eng, tmp_path):
    """`--segmentation 0:50` in `scrappie seqmappy` and `scrappie mappy` leaves the variance-based segmentation out, as it does in
    `scrappie events`: the read's window is [200, n - 10), and the output is that of the same window, normalised by the Python
    surface, through Engine.map_to_sequence / Engine.mappy"""
    name = list(FA_SHA256)[0]
    fa, f5 = os.path.join(READS, name + ".fa"), os.path.join(READS, "read_ch228_file118.i16")
    seq = _fasta(name)
    raw = sa.read_raw(f5)[0]
    n = len(raw)
    rt = sa.RawTable(raw, 200, n - 10).scale()
    x = rt._data                                           # the window normalised in place, the trims as they were read
    mfile = str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(model.synthetic_model("rgrgr_r94", seed=1), mfile)
    (score, path), = eng.map_to_sequence([rt], [seq], viterbi=True, path=True, stay_pen=0.0, skip_pen=0.0, local_pen=4.0, min_prob=1e-5)
    want = "# %s to %s -- score %f over %d blocks (%f per block)\nblock\tpos\n" % (f5, fa, -score, len(path), np.float32(-score) / np.float32(len(path)))
    want += "".join("%d\t%d\n" % (i, p) for i, p in enumerate(path))
    r = subprocess.run([CLI, "seqmappy", "--model-file", mfile, "--segmentation", "0:50", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want

    sfile = str(tmp_path / "squiggle_r94.scrm")
    model.save_model(model.synthetic_model("squiggle_r94", seed=11), sfile)
    eng.load_model("squiggle_r94", sfile)
    (score, path), = eng.mappy([rt], [seq])
    sq = eng.predict_squiggle([seq], model="squiggle_r94", rescale=False)[0]
    libm = C.CDLL("libm.so.6")
    libm.expf.restype, libm.expf.argtypes = C.c_float, [C.c_float]
    want = ["# %s to %s  (score = %f)" % (f5, fa, score), "idx\tsignal\tpos\tbase\tcurrent\tsd\tdwell"]
    assert len(path) == n
    for i, p in enumerate(path):
        if p >= 0:
            want.append("%d\t%3.6f\t%d\t%s\t%3.6f\t%3.6f\t%3.6f" % (i, x[i], p, seq[p], sq[p, 0], libm.expf(sq[p, 1]), libm.expf(-sq[p, 2])))
        else:
            want.append("%d\t%3.6f\t%d\tN\tnan\tnan\tnan" % (i, x[i] if 200 <= i < n - 10 else float("nan"), p))
    r = subprocess.run([CLI, "mappy", "--model-file", sfile, "--segmentation", "0:50", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == want


def test_per_read_threads():
    cases = [c for c in map_cases(big=False) if c[1].shape[0] == 800][:16]
    L = sa.lib()
    alone = [call_map(L, post, seq, pens, True, cast=PM) for _, post, seq, pens in cases]
    with ThreadPoolExecutor(16) as ex:
        together = list(ex.map(lambda c: call_map(L, c[1], c[2], c[3], True, cast=PM), cases))
    for (a_s, a_p), (t_s, t_p) in zip(alone, together):
        assert a_s.tobytes() == t_s.tobytes() and np.array_equal(a_p, t_p)


def _small_call(n, seed):
    """n reads of 600 to 1000 samples with a sequence of 30 states (34 bases) each"""
    rng = np.random.default_rng(seed)
    sigs = [synth.medmad_normalise(synth.synthetic_signal(int(k), 500 + i)) for i, k in enumerate(rng.integers(600, 1000, n))]
    return sigs, [_bases(34, rng) for _ in sigs]


def _same_results(a, b, skip=()):
    assert len(a) == len(b)
    for i, ((sa_, pa), (sb, pb)) in enumerate(zip(a, b)):
        if i in skip:
            continue
        assert np.float32(sa_).tobytes() == np.float32(sb).tobytes(), (i, sa_, sb)
        assert (pa is None and pb is None) or np.array_equal(pa, pb), i


def test_engine_map_cut_by_memory(eng):
    """launch groups cut by device bytes, not by reads: a budget of 240 column blocks.  A group costs
    (sum T / 16 + max T + 1) blocks + under one block of traceback and codes, T the reads' blocks (samples / 5):
    T = 200, 140, [300], 198 | 200, 120, 199 | 170 -- the fourth read would make 247 and 244 -- and the read of 300 blocks
    needs 319 alone: refused.  The others as in one uncut launch group, bit for bit."""
    lens = [1000, 700, 1500, 990, 1000, 600, 995, 850]
    rng = np.random.default_rng(51)
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 400 + i)) for i, n in enumerate(lens)]
    seqs = [_bases(34, rng) for _ in lens]
    assert [eng.read_blocks("rgrgr_r94", n) for n in lens] == [200, 140, 300, 198, 200, 120, 199, 170]
    kw = dict(viterbi=True, path=True, stay_pen=0.5, skip_pen=1.0, local_pen=4.0)
    form = (True, False, True, False)                      # Viterbi, unbanded, tiled, LDS: one launch per group
    before = sa.launch_form_counts()["map"][form]
    uncut = eng.map_to_sequence(sigs, seqs, **kw)
    assert sa.launch_form_counts()["map"][form] == before + 1
    assert all(np.isfinite(sc) and pth is not None for sc, pth in uncut)
    eng.set_max_launch_blocks(240)
    try:
        cut = eng.map_to_sequence(sigs, seqs, **kw)
        err = sa.last_error()
    finally:
        eng.set_max_launch_blocks(0)
    groups = sa.launch_form_counts()["map"][form] - before - 1
    print("launch groups under a budget of 240 blocks: %d" % groups)
    assert groups >= 3
    assert np.isnan(cut[2][0]) and cut[2][1] is None
    assert "read 2" in err and "too long for one launch group" in err, err
    _same_results(cut, uncut, skip=(2,))


def test_engine_failed_launch_group(eng):
    """the second of three launch groups refused (debug option fail_run): the call fails with that text and hands nothing
    back, and the engine then gives what it gave before"""
    sigs, seqs = _small_call(40, 61)
    kw = dict(viterbi=True, path=True, stay_pen=0.5, skip_pen=1.0, local_pen=4.0)
    form = (True, False, True, False)
    eng.set_max_launch_reads(16)
    try:
        before = sa.launch_form_counts()["map"][form]
        first = eng.map_to_sequence(sigs, seqs, **kw)
        assert sa.launch_form_counts()["map"][form] - before == 3
        assert all(np.isfinite(sc) and pth is not None for sc, pth in first)
        eng.debug_option("fail_run", 2)
        got = None
        with pytest.raises(RuntimeError, match="injected failure"):
            got = eng.map_to_sequence(sigs, seqs, **kw)
        assert got is None
        assert sa.launch_form_counts()["map"][form] - before == 4          # the first group ran, the second was refused, no third
        eng.debug_option("fail_run", 0)
        _same_results(eng.map_to_sequence(sigs, seqs, **kw), first)
    finally:
        eng.debug_option("fail_run", 0)
        eng.set_max_launch_reads(16384)


def test_debug_fetch_tile_boff(eng):
    """the launch group's stored first column block per tile is the running sum of the tiles' longest reads"""
    lens = [600 + 37 * i for i in range(20)]               # two tiles
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 700 + i)) for i, n in enumerate(lens)]
    rng = np.random.default_rng(71)
    assert all(np.isfinite(sc) for sc, _ in eng.map_to_sequence(sigs, [_bases(34, rng) for _ in sigs]))      # one launch group
    order = eng.debug_fetch("order", np.int32)
    got = eng.debug_fetch("tile_boff", np.int64)
    assert len(order) == 32 and sorted(o for o in order if o >= 0) == list(range(20))
    T = [eng.read_blocks("rgrgr_r94", n) for n in lens]
    tile_T = [max(T[o] if o >= 0 else 0 for o in order[t * 16:(t + 1) * 16]) for t in range(2)]
    assert tile_T[0] > 0 and tile_T[1] > 0
    assert got.tolist() == [0, tile_T[0]]


def test_every_map_form_was_launched(forms_at_start):
    """the last test of the module: each of the 16 k_map instantiations (Viterbi / forward x full / banded x dense / tiled
    x LDS / scratch) has been launched by the tests above"""
    now = sa.launch_form_counts()["map"]
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("k_map launches by (viterbi, banded, tiled, scratch): %r" % sorted(ran.items()))
    assert len(ran) == 16 and all(v > 0 for v in ran.values()), ran
