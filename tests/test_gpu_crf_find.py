"""k_crf_find on the device (csrc/sh_crf_find.h): the per-read symbol against the float32 restatement np_crf_find in bits -- score,
begin, end and call_score -- over read lengths, motif lengths and pack shapes; the score of a motif does not depend on the pack
size; the batched engine against the per-read function on the same transitions; the command line.  The last test requires all
four kernel forms (positions x loader) to have been launched by this module."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_crf_find_cpu import bits, check_find, np_crf_find
from test_gpu_map_crf import READ, READS, _HostMat, _prepared
from test_map_crf_cpu import _trans, call_of, np_decode_crf, np_map_crf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
NBLOCKS = (1, 2, 3, 17, 64, 65)


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """k_crf_find launches per form before this module's first test (test_every_crf_find_form_was_launched)"""
    return sa.crf_find_form_counts()


@pytest.fixture(autouse=True)
def default_cells():
    yield
    sa.set_crf_find_cells(-1)


def maxc():
    return sa.crf_find_max_cells()


def gpu_find(trans, motifs, positions=True, cells=-1, mat_stride=28):
    """the per-read symbol at a pack size: (scores, call_score, begins, ends, return code, error text)"""
    sa.set_crf_find_cells(cells)
    m = _HostMat(np.ascontiguousarray(trans, dtype=np.float32), mat_stride)
    n = len(motifs)
    keep = [np.ascontiguousarray(x, dtype=np.int32) for x in motifs]
    tgs = (sa._MapTarget * max(n, 1))()
    for i, cd in enumerate(keep):
        tgs[i].seq = cd.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(cd)
    score = np.full(max(n, 1), 123.0, dtype=np.float32)
    begin, end = np.full(max(n, 1), -7, dtype=np.int32), np.full(max(n, 1), -7, dtype=np.int32)
    call = C.c_float(123.0)
    i32 = C.POINTER(C.c_int32)
    rc = sa.lib().find_crf_sequences_viterbi(C.byref(m.mat), tgs, n, score.ctypes.data_as(C.POINTER(C.c_float)),
                                             begin.ctypes.data_as(i32) if positions else None, end.ctypes.data_as(i32) if positions else None,
                                             C.byref(call))
    return score[:n], np.float32(call.value), (begin[:n] if positions else None), (end[:n] if positions else None), rc, sa.last_error()


def against_restatement(trans, motifs, want=None, tag="", **kw):
    """score, begin, end and call_score in bits; returns the restatement's results (computed once per set: pass them back as `want`)"""
    if want is None:
        want = [np_crf_find(trans, mo) for mo in motifs]
    sc, call, bg, en, rc, err = gpu_find(trans, motifs, **kw)
    assert rc == 0, err
    for k, w in enumerate(want):
        if np.isnan(w["score"]):
            assert np.isnan(sc[k]) and (bg is None or (bg[k], en[k]) == (-1, -1)), (tag, k, sc[k])
            continue
        assert bits(sc[k]) == bits(w["score"]), (tag, k, sc[k], w["score"])
        if bg is not None:
            assert (int(bg[k]), int(en[k])) == (w["begin"], w["end"]), (tag, k, bg[k], en[k], w["begin"], w["end"])
    if want:
        assert bits(call) == bits(want[0]["call_score"]), (tag, call, want[0]["call_score"])
    return want


# ---------------------------------------------------------------------------
# the per-read symbol
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nblock", NBLOCKS)
def test_grid_against_restatement(nblock):
    rng = np.random.default_rng(100 + nblock)
    for sigma in (0.5, 3.0):
        trans = _trans(nblock, sigma, rng)
        lens = sorted(set(min(x, maxc() - 9) for x in (1, 2, 3, nblock, nblock + 1, nblock + 2)))
        motifs = [rng.integers(0, 4, L) for L in lens]
        motifs += [np.full(L, b) for b, L in ((0, 1), (1, 2), (2, min(5, nblock + 1)), (3, nblock + 1))]      # homopolymers
        ds, dp = np_decode_crf(trans)
        seq, _ = call_of(dp)
        if len(seq):
            motifs += [seq, seq[len(seq) // 2:len(seq) // 2 + 3]]                                         # runs of the call
        want = against_restatement(trans, motifs, tag="n%d s%g" % (nblock, sigma))
        assert bits(want[0]["call_score"]) == bits(ds)
        for mo, w in zip(motifs, want):
            if not np.isnan(w["score"]):
                check_find(trans, mo, w)
        if len(seq):
            assert bits(want[-1]["score"]) == bits(ds) and bits(want[-2]["score"]) == bits(ds)
        assert np.isnan(want[lens.index(nblock + 2)]["score"])
        against_restatement(trans, motifs, want=want, positions=False, mat_stride=25, tag="no positions")
        g, _ = np_map_crf(trans, motifs[lens.index(nblock + 1)])                                           # the only path
        assert bits(want[lens.index(nblock + 1)]["score"]) == bits(g)
    sc, call, bg, en, rc, err = gpu_find(trans, [rng.integers(0, 4, nblock + 2), [1]])
    assert rc == 0 and np.isnan(sc[0]) and np.isfinite(sc[1]) and "motif 0" in err and "no occurrence" in err, err


def test_all_zero_matrix():
    """the tie order, as tests/test_crf_find_cpu.py works it out by hand for NB = 3"""
    z = np.zeros((3, 25), dtype=np.float32)
    sc, call, bg, en, rc, err = gpu_find(z, [[2], [1, 3]])
    assert rc == 0, err
    assert [bits(x) for x in sc] == [bits(0.0)] * 2 and bits(call) == bits(0.0)
    assert (list(bg), list(en)) == ([0, 0], [0, 1])
    z = np.zeros((20, 25), dtype=np.float32)
    against_restatement(z, [[0], [3, 3, 3], [0, 1, 2, 3, 0, 1, 2], list(range(4)) * 5 + [0], [2] * 22], tag="zero")


def _forty(rng, k):
    return [rng.integers(0, 4, 40) for _ in range(k)]


def pack_sets(rng):
    """name -> motifs.  A motif of L bases takes L + 4 cells behind the pack's 5: k motifs of 40 bases and a filler make the cell counts"""
    out = {"1": [rng.integers(0, 4, 9)], "2": [rng.integers(0, 4, 30), rng.integers(0, 4, 1)],
           "7": [rng.integers(0, 4, L) for L in (1, 40, 2, 17, 1, 33, 40)]}
    for cells, k in ((255, 5), (256, 5), (257, 5), (513, 11)):
        fill = cells - 5 - 44 * k - 4
        ms = _forty(rng, k) + [rng.integers(0, 4, fill)]
        assert 5 + sum(len(x) + 4 for x in ms) == cells
        out["cells-%d" % cells] = ms
    out["three-packs-at-128"] = _forty(rng, 5)
    assert sa.crf_find_plan([40] * 5, 128)[0] == 3
    return out


def test_pack_shapes_and_pack_sizes_give_the_same_bits():
    rng = np.random.default_rng(77)
    trans = _trans(48, 2.0, rng)
    ds, dp = np_decode_crf(trans)
    for name, motifs in pack_sets(rng).items():
        want = None
        for cells in (maxc(), 64, 128, -1):
            want = against_restatement(trans, motifs, want=want, cells=cells, tag="%s at %d" % (name, cells))
        against_restatement(trans, motifs, want=want, cells=128, positions=False, tag=name + " without positions")


def test_the_longest_motif_and_one_too_long():
    """max_cells() - 9 bases fill the LDS alone; one base more is refused with the text, its neighbours are scored"""
    rng = np.random.default_rng(9)
    L = maxc() - 9
    trans = _trans(L + 6, 2.0, rng)
    motifs = [rng.integers(0, 4, 12), rng.integers(0, 4, L), rng.integers(0, 4, L + 1), rng.integers(0, 4, 3)]
    want = [np_crf_find(trans, mo) for mo in (motifs[0], motifs[1], motifs[3])]
    assert all(np.isfinite(w["score"]) for w in want)
    for pos in (True, False):
        sc, call, bg, en, rc, err = gpu_find(trans, motifs, positions=pos)
        assert rc == 0 and "motif 2" in err and "too long for k_crf_find" in err, err
        assert np.isnan(sc[2]) and (not pos or (bg[2], en[2]) == (-1, -1))
        for k, w in zip((0, 1, 3), want):
            assert bits(sc[k]) == bits(w["score"]), k
            assert not pos or (int(bg[k]), int(en[k])) == (w["begin"], w["end"]), k
        assert bits(call) == bits(want[0]["call_score"])


def test_bad_motifs_per_read():
    trans = _trans(30, 2.0, np.random.default_rng(2))
    good = against_restatement(trans, [[0, 1, 2], [3]])
    sc, call, bg, en, rc, err = gpu_find(trans, [[0, 1, 2], [0, 4, 1], [3], []])
    assert rc == 0 and "motif 1" in err and "not a base" in err, err
    assert np.isnan(sc[1]) and np.isnan(sc[3]) and bits(sc[0]) == bits(good[0]["score"]) and bits(sc[2]) == bits(good[1]["score"])
    sc, call, bg, en, rc, err = gpu_find(trans, [])                        # no motifs: the call score alone
    assert rc == 0 and bits(call) == bits(good[0]["call_score"])
    m = sa.ScrappyMatrix.from_numpy(trans, sloika=False)
    s, c, b, e = sa.find_in_trans(m, ["ACG", "T"])
    assert [bits(x) for x in s] == [bits(w["score"]) for w in good] and bits(c) == bits(good[0]["call_score"])
    assert list(b) == [w["begin"] for w in good] and list(e) == [w["end"] for w in good]
    s2, c2, b2, e2 = sa.find_in_trans(m, ["ACG", "T"], positions=False)
    assert b2 is None and e2 is None and s2.tobytes() == s.tobytes()


# ---------------------------------------------------------------------------
# the batched engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    return model.synthetic_model("rnnrf_r94", seed=11), model.synthetic_model("rgrgr_r94", seed=1)


@pytest.fixture(scope="module")
def eng(weights):
    e = sa.Engine(0)
    e.load_model("rnnrf_r94", weights[0])
    e.load_model("rgrgr_r94", weights[1])
    yield e
    e.close()


def _sig(n, seed):
    return synth.medmad_normalise(synth.synthetic_signal(n, seed))


def _str(codes):
    return "".join("ACGT"[b] for b in codes)


@pytest.fixture(scope="module")
def call(eng):
    """18 reads of 1000 .. 4000 samples (two tiles, the second nearly empty), their transitions and calls (the bases of all
    nblock + 1 entries of decode_crf's path), a shared list of motifs and one list per read with pieces of the read's own call"""
    rng = np.random.default_rng(41)
    lens = [int(x) for x in rng.integers(1000, 4000, 18)]
    sigs = [_sig(n, 700 + i) for i, n in enumerate(lens)]
    trans = [eng.posterior(x, "rnnrf_r94") for x in sigs]
    calls = [call_of(np_decode_crf(t)[1])[0] for t in trans]
    shared = [_str(rng.integers(0, 4, 40)) for _ in range(6)] + [_str(rng.integers(0, 4, 24)) for _ in range(3)] + ["G"]
    own = []
    for c in calls:
        L = len(c)
        ms = [_str(rng.integers(0, 4, 24))]
        if L >= 12:
            ms += [_str(c[L // 3:L // 3 + 8]), _str(c[2:min(L - 2, 42)]), _str(c[L // 2:L // 2 + 1])]
        own.append(ms + [_str(rng.integers(0, 4, 40))])
    return dict(sigs=sigs, lens=lens, trans=trans, calls=calls, shared=shared, own=own)


def _check_against_per_read(call, lists, res, positions=True, skip=()):
    for i, (sc, cs, best, bg, en) in enumerate(res):
        if i in skip:
            continue
        motifs = [sa.encode_bases(m, 1).astype(np.int32) for m in lists[i]]
        ws, wc, wb, we, rc, err = gpu_find(call["trans"][i], motifs, positions=positions)
        assert rc == 0, err
        assert sc.tobytes() == ws.tobytes() and bits(cs) == bits(wc), (i, sc, ws)
        assert np.all(np.isfinite(sc)) and best == int(np.argmax(sc)), i
        if positions:
            assert np.array_equal(bg, wb) and np.array_equal(en, we), i
        else:
            assert bg is None and en is None


def test_engine_find_sequences(eng, call):
    n = len(call["sigs"])
    res = eng.find_sequences(call["sigs"], call["shared"])
    _check_against_per_read(call, [call["shared"]] * n, res)
    same = eng.find_sequences(call["sigs"], [list(call["shared"]) for _ in range(n)])             # a shared list and per-read lists agree
    for a, b in zip(res, same):
        assert a[0].tobytes() == b[0].tobytes() and bits(a[1]) == bits(b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    nopos = eng.find_sequences(call["sigs"], call["shared"], positions=False)
    _check_against_per_read(call, [call["shared"]] * n, nopos, positions=False)
    t = eng.map_timing()
    assert t["network_ms"] > 0 and t["map_ms"] > 0
    # pieces of a read's own call: the call's score, bit for bit
    res = eng.find_sequences(call["sigs"], call["own"])
    _check_against_per_read(call, call["own"], res)
    nown = 0
    for i, (sc, cs, best, bg, en) in enumerate(res):
        assert bits(cs) == bits(np_decode_crf(call["trans"][i])[0]), i
        assert np.all(sc <= cs), i
        for k in range(1, len(call["own"][i]) - 1):
            nown += 1
            assert bits(sc[k]) == bits(cs), (i, k, sc[k], cs)
            assert 0 <= bg[k] <= en[k] <= eng.read_blocks("rnnrf_r94", call["lens"][i])
    print("pieces of the reads' own calls: %d" % nown)
    assert nown >= 3


def test_engine_several_launch_groups(eng, call):
    """the same call under a budget of 900 column blocks: at least three launch groups, the same bits"""
    uncut = eng.find_sequences(call["sigs"], call["own"])
    before = sa.crf_find_form_counts()[(True, True)]
    eng.set_max_launch_blocks(900)
    try:
        cut = eng.find_sequences(call["sigs"], call["own"])
    finally:
        eng.set_max_launch_blocks(0)
    groups = sa.crf_find_form_counts()[(True, True)] - before
    print("launch groups under a budget of 900 blocks: %d" % groups)
    assert groups >= 3
    for i, (a, b) in enumerate(zip(uncut, cut)):
        assert a[0].tobytes() == b[0].tobytes() and bits(a[1]) == bits(b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), i
    eng.debug_option("crf_find_cells", 128)                                     # another pack size on the engine: the same bits
    try:
        other = eng.find_sequences(call["sigs"], call["own"])
    finally:
        eng.debug_option("crf_find_cells", -1)
    for i, (a, b) in enumerate(zip(uncut, other)):
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), i


def test_engine_refusals_leave_neighbours_untouched(eng, call):
    sigs = list(call["sigs"][:6])
    lists = [list(x) for x in call["own"][:6]]
    good = eng.find_sequences(sigs, lists)
    lists[1][0] = "ACGTNACGT"                              # not a base
    lists[2][1] = "A" * (maxc() - 8)                       # too long for k_crf_find
    sigs[4] = _sig(5, 1)                                   # a read too short for the model
    res = eng.find_sequences(sigs, lists)
    err = sa.last_error()
    assert "read 1" in err and "motif 0" in err, err
    assert np.isnan(res[1][0][0]) and res[1][0][1:].tobytes() == good[1][0][1:].tobytes() and res[1][3][0] == -1
    assert np.isnan(res[2][0][1]) and res[2][0][2:].tobytes() == good[2][0][2:].tobytes() and bits(res[2][0][0]) == bits(good[2][0][0])
    assert np.all(np.isnan(res[4][0])) and len(res[4][0]) == len(lists[4]) and res[4][2] == -1
    for i in (0, 3, 5):
        assert res[i][0].tobytes() == good[i][0].tobytes() and res[i][2] == good[i][2] and np.array_equal(res[i][3], good[i][3]), i
    res = eng.find_sequences(sigs[2:3], lists[2:3])
    assert "too long for k_crf_find" in sa.last_error()
    res = eng.find_sequences(sigs[4:5], lists[4:5])
    assert "too short" in sa.last_error() and res[0][2] == -1


def test_transducer_model_is_refused(eng, call):
    with pytest.raises(RuntimeError, match="rgrgr_r94.*transducer"):
        eng.find_sequences(call["sigs"][:2], ["ACGTACGTAC"], model="rgrgr_r94")
    assert "find_batch" in sa.last_error()


def test_seqmappy_find_cli(eng, weights, tmp_path):
    """`scrappie seqmappy --model rnnrf_r94 --find` on a bundled read and a FASTA of motifs: what Engine.find_sequences gives; the
    refusals name the option and print nothing"""
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    seq, _ = call_of(np_decode_crf(eng.posterior(x, "rnnrf_r94"))[1])
    assert len(seq) >= 1
    rng = np.random.default_rng(8)
    recs = [("own_a", _str(seq[len(seq) // 4:len(seq) // 4 + 24])), ("random40", _str(rng.integers(0, 4, 40))), ("own_b", _str(seq[len(seq) // 2:len(seq) // 2 + 40])),
            ("not_bases", "ACGTNNACGT"), ("one", "T")]
    fa = str(tmp_path / "motifs.fa")
    with open(fa, "w") as fh:
        fh.write("".join(">%s\n%s\n" % r for r in recs))
    crf_file, tr_file = str(tmp_path / "rnnrf_r94.scrm"), str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(weights[0], crf_file)
    model.save_model(weights[1], tr_file)
    (sc, cs, best, bg, en), = eng.find_sequences([x], [r[1] for r in recs])
    nblock = eng.read_blocks("rnnrf_r94", len(x))
    assert bits(sc[0]) == bits(cs) and bits(sc[2]) == bits(cs) and np.isnan(sc[3]) and best == 0
    want = "# %s to %s -- %d records, call score %f over %d blocks, best %d\nrecord\tname\tscore\tdelta\tbegin\tend\n" % (f5, fa, len(recs), cs, nblock, best)
    for k, (name, _) in enumerate(recs):
        if np.isnan(sc[k]):
            want += "%d\t%s\tnan\tnan\t-1\t-1\n" % (k, name)
        else:
            want += "%d\t%s\t%f\t%f\t%d\t%d\n" % (k, name, sc[k], np.float32(sc[k]) - np.float32(cs), bg[k], en[k])
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--find", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    # the refusals name the option
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--find", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--find" in r.stderr and r.stdout == ""
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--find", "--inside", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--find" in r.stderr and "--inside" in r.stderr and r.stdout == ""
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--find", "--all-records", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--find" in r.stderr and "--all-records" in r.stderr and r.stdout == ""
    u = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    assert "--find" in u.stderr + u.stdout


def test_every_crf_find_form_was_launched(forms_at_start):
    """the last test of the module: each of the 4 k_crf_find instantiations (positions or not x reference layout / tiled) has been
    launched by the tests above"""
    now = sa.crf_find_form_counts()
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("k_crf_find launches by (positions, tiled): %r" % sorted(ran.items()))
    assert len(ran) == 4 and all(v > 0 for v in ran.values()), ran
