"""Reads of a flip-flop (CRF) model mapped INTO a longer base sequence on the GPU (k_map_crf_local, sh_map_crf_local.h): the
per-read symbols against the numpy restatement of tests/test_map_crf_local_cpu.py at every stride and in both homes and, on the
cases made from a call, against the compiled reference's decode_crf (oracle/_ref/libref_decode.so); scrappie_hip_map_local_batch /
Engine.map_to_reference against the per-read symbols on the read's own transitions; `scrappie seqmappy --inside`.  Viterbi scores,
first, last and paths are bit-identical (on ties: the score, and a path that passes the checker); forward scores lie within
|gpu - f64| <= 2 |np32 - f64| + 1e-5 |f64|, the float32 restatement making the same cut and the same order of reduction."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_gpu_map_crf import READ, READS, _HostMat, _ip, _prepared, _same_bits
from test_map_crf_cpu import _trans, call_of, map_crf_cases, np_map_crf, ref_decode_crf
from test_map_crf_local_cpu import check_local_path, embed, max_cells, np_map_crf_local

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
NBLOCKS = (1, 2, 5, 63, 64, 65)
LENGTHS = (1, 2, 63, 64, 65, 300, 1000)
STRIDES = (1, 7, 64, -1, 0)


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """k_map_crf_local launches per form before this module's first test (test_every_map_crf_local_form_was_launched)"""
    return sa.map_crf_local_form_counts()


@pytest.fixture(scope="module")
def worst():
    """the worst forward ratio |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) the module has seen, printed by its last test"""
    return dict(lds=0.0, scratch=0.0)


@pytest.fixture(autouse=True)
def default_stride():
    yield
    sa.set_map_crf_local_stride(-1)


def gpu_local(trans, seq, viterbi=True, stride=-1, mat_stride=28, want=True):
    """one per-read symbol at a stride of the window cut: (float32 score, first, last, path)"""
    L = sa.lib()
    sa.set_map_crf_local_stride(stride)
    m = _HostMat(np.ascontiguousarray(trans, dtype=np.float32), mat_stride)
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    if not viterbi:
        return np.float32(L.map_crf_to_reference_forward(C.byref(m.mat), _ip(seq), len(seq))), None, None, None
    path = np.full(trans.shape[0] + 1, -7, dtype=np.int32)
    first, last = C.c_size_t(12345), C.c_size_t(12345)
    s = L.map_crf_to_reference_viterbi(C.byref(m.mat), _ip(seq), len(seq), C.byref(first) if want else None, C.byref(last), _ip(path) if want else None)
    return np.float32(s), (int(first.value) if want else None), int(last.value), (path if want else None)


def _forward_ok(got, np32, f64, worst, key):
    eg, er = abs(float(got) - float(f64)), abs(float(np32) - float(f64))
    print("forward: gpu %.9g np32 %.9g f64 %.12g" % (got, np32, f64))
    assert eg <= 2 * er + 1e-5 * abs(float(f64)), (got, np32, f64)
    worst[key] = max(worst[key], eg / (2 * er + 1e-5 * abs(float(f64)) + 1e-30))


@pytest.fixture(scope="module")
def grid():
    """one matrix per nblock and one sequence per L, and the one-window restatement of every pair, computed once"""
    rng = np.random.default_rng(77)
    trans = {nb: _trans(nb, 2.0, rng) for nb in NBLOCKS}
    seqs = {L: rng.integers(0, 4, L).astype(np.int32) for L in LENGTHS}
    want = {(nb, L): np_map_crf_local(trans[nb], seqs[L]) for nb in NBLOCKS for L in LENGTHS}
    return dict(trans=trans, seqs=seqs, want=want)


@pytest.mark.parametrize("nblock", NBLOCKS)
def test_viterbi_grid_against_restatement(nblock, grid):
    """score, first, last and path in bits at strides 1, 7, 64, the default and one window: the one-window restatement's"""
    tr = grid["trans"][nblock]
    for L in LENGTHS:
        seq = grid["seqs"][L]
        ws, wf, wl, wp = grid["want"][(nblock, L)]
        check_local_path(tr, seq, ws, wf, wl, wp)
        for stride in STRIDES:
            gs, gf, gl, gp = gpu_local(tr, seq, stride=stride, mat_stride=25 if stride == 7 else 28)
            assert _same_bits(gs, ws), (nblock, L, stride, gs, ws)
            assert (gf, gl) == (wf, wl) and np.array_equal(gp, wp), (nblock, L, stride, gf, gl, wf, wl)
        gs, gf, gl, gp = gpu_local(tr, seq, want=False)          # no path wanted: the first pass alone
        assert _same_bits(gs, ws) and gl == wl and gf is None and gp is None


@pytest.mark.parametrize("nblock", (1, 5, 64, 65))
def test_forward_grid_against_restatement(nblock, grid, worst):
    tr = grid["trans"][nblock]
    for L in LENGTHS:
        seq = grid["seqs"][L]
        f64 = np_map_crf_local(tr, seq, viterbi=False, dtype=np.float64)[0]
        for stride in STRIDES:
            if (stride == 1 and L > 65) or (stride == 7 and L > 300):
                continue                                         # (the restatement walks the windows one by one)
            n32 = np_map_crf_local(tr, seq, stride=stride, viterbi=False)[0]
            _forward_ok(gpu_local(tr, seq, viterbi=False, stride=stride)[0], n32, f64, worst, "lds")


def test_lds_windows_and_one_scratch_window_agree(worst):
    """L = 4000, nblock = 40: the default stride (windows in LDS) and stride 0 (one window of 4001 cells, in scratch)"""
    rng = np.random.default_rng(78)
    tr, seq = _trans(40, 2.0, rng), rng.integers(0, 4, 4000).astype(np.int32)
    assert 4001 > max_cells() and not sa.map_crf_local_plan(4000, 40, -1)["home"].any() and sa.map_crf_local_plan(4000, 40, 0)["home"].tolist() == [1]
    ws, wf, wl, wp = np_map_crf_local(tr, seq)
    check_local_path(tr, seq, ws, wf, wl, wp)
    f64 = np_map_crf_local(tr, seq, viterbi=False, dtype=np.float64)[0]
    for stride, scr in ((-1, False), (0, True)):
        before = sa.map_crf_local_form_counts()
        gs, gf, gl, gp = gpu_local(tr, seq, stride=stride)
        after = sa.map_crf_local_form_counts()
        assert after[(True, False, scr)] - before[(True, False, scr)] == 2 and after[(True, False, not scr)] == before[(True, False, not scr)]
        assert _same_bits(gs, ws) and (gf, gl) == (wf, wl) and np.array_equal(gp, wp), (stride, gs, ws)
        n32 = np_map_crf_local(tr, seq, stride=stride, viterbi=False)[0]
        _forward_ok(gpu_local(tr, seq, viterbi=False, stride=stride)[0], n32, f64, worst, "scratch" if scr else "lds")
        assert sa.map_crf_local_form_counts()[(False, False, scr)] == after[(False, False, scr)] + 1


def test_tie_cases():
    """a homopolymer reference and the all-zero matrix: the score in bits and a path that passes the checker"""
    rng = np.random.default_rng(79)
    for tr, seq in ((_trans(40, 2.0, rng), np.full(90, 2)), (np.zeros((12, 25), dtype=np.float32), rng.integers(0, 4, 40)),
                    (np.zeros((9, 25), dtype=np.float32), np.full(5, 1)), (np.zeros((70, 25), dtype=np.float32), np.full(300, 3))):
        seq = seq.astype(np.int32)
        ws = np_map_crf_local(tr, seq)[0]
        for stride in STRIDES:
            gs, gf, gl, gp = gpu_local(tr, seq, stride=stride)
            assert _same_bits(gs, ws), (stride, gs, ws)
            check_local_path(tr, seq, gs, gf, gl, gp)


def test_embedding_identity_against_decode_crf():
    """flank + call + flank on the fixture calls: decode_crf's score in bits (the compiled reference's), first, last, its path
    shifted; and never below the global mapping of the same pair"""
    assert ref_decode_crf(np.zeros((1, 25), np.float32)) is not None, "oracle/_ref/libref_decode.so is required (build() makes it and it travels with the tree)"
    rng = np.random.default_rng(101)
    n = 0
    for c in map_crf_cases():
        if not c["from_call"]:
            continue
        ds, dp = ref_decode_crf(c["trans"])
        seq, path = call_of(dp)
        for nl, nr in ((0, 0), (1, 1), (37, 37)):
            ref, at = embed(c, nl, nr, rng)
            for stride in (-1, 7):
                gs, gf, gl, gp = gpu_local(c["trans"], ref, stride=stride)
                assert _same_bits(gs, ds), (c["name"], nl, nr, stride, gs, ds)
                assert (gf, gl) == (at, at + len(seq)) and np.array_equal(gp, path + at), (c["name"], nl, nr, stride)
            n += 1
    assert n == 72
    for c in map_crf_cases():
        g = np_map_crf(c["trans"], c["seq"])[0]
        gs, gf, gl, gp = gpu_local(c["trans"], c["seq"])
        check_local_path(c["trans"], c["seq"], gs, gf, gl, gp)
        assert np.isnan(g) or gs >= np.float32(g), c["name"]


def test_refusals_per_read():
    L = sa.lib()
    tr = np.zeros((4, 25), dtype=np.float32)
    seq = np.array([0, 1, 2, 3, 0, 1, 2], dtype=np.int32)
    m = _HostMat(tr)
    assert np.isnan(L.map_crf_to_reference_viterbi(None, _ip(seq), 7, None, None, None)) and "null" in sa.last_error()
    assert np.isnan(L.map_crf_to_reference_forward(C.byref(m.mat), None, 7)) and "null" in sa.last_error()
    assert np.isfinite(L.map_crf_to_reference_viterbi(C.byref(m.mat), _ip(seq), 7, None, None, None))
    bad = _HostMat(tr)
    bad.mat.nr = 24
    assert np.isnan(L.map_crf_to_reference_forward(C.byref(bad.mat), _ip(seq), 7)) and "25 rows" in sa.last_error()
    for code in (4, -1):
        s2 = seq.copy()
        s2[5] = code
        assert np.isnan(L.map_crf_to_reference_viterbi(C.byref(m.mat), _ip(s2), 7, None, None, None)) and "not a base" in sa.last_error()
    assert np.isnan(L.map_crf_to_reference_forward(C.byref(m.mat), _ip(seq), 0)) and "empty" in sa.last_error()


def test_scrappy_style_map_trans_to_reference():
    c = {x["name"]: x for x in map_crf_cases()}["call-s2-n200"]
    ref, at = embed(c, 50, 60, np.random.default_rng(3))
    m = sa.ScrappyMatrix.from_numpy(c["trans"], sloika=False)
    bases = "".join("ACGT"[b] for b in ref)
    s, first, last, p = sa.map_trans_to_reference(m, bases, viterbi=True, path=True)
    assert _same_bits(s, c["dscore"]) and (first, last) == (at, at + len(c["seq"])) and np.array_equal(p, c["dpath"] + at)
    s, first, last, p = sa.map_trans_to_reference(m, bases, viterbi=True)
    assert _same_bits(s, c["dscore"]) and first is None and last == at + len(c["seq"]) and p is None
    s, first, last, p = sa.map_trans_to_reference(m, bases)
    f64 = np_map_crf_local(c["trans"], ref, viterbi=False, dtype=np.float64)[0]
    assert p is None and abs(s - f64) < 1e-3 * abs(f64) and s >= c["dscore"]


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


def _batch(eng, sigs, codes, vit=True, path=True):
    """scrappie_hip_map_local_batch itself: codes[i] an int32 array (the same object for reads that share a sequence).
    Returns ([(score, first, last, path)], return code, error text)"""
    n = len(sigs)
    rts, keep = sa._raw_tables(sigs)
    tgs = (sa._MapLocalTarget * n)()
    for i, cd in enumerate(codes):
        tgs[i].seq = cd.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(cd)
    out = (sa._MapLocalResult * n)()
    rc = sa.lib().scrappie_hip_map_local_batch(eng._h, eng._models["rnnrf_r94"], rts, tgs, n, None, 1 if vit else 0, 1 if path else 0, out)
    err = sa.last_error()
    res = []
    for r in (out[i] for i in range(n)):
        pth = np.ctypeslib.as_array(r.path, shape=(r.nblock + 1,)).copy() if r.path else None
        res.append((np.float32(r.score), int(r.first), int(r.last), pth))
    sa.lib().scrappie_hip_free_map_local_results(out, n)
    return res, rc, err


@pytest.fixture(scope="module")
def call(eng):
    """18 reads of ragged lengths (two tiles, the second nearly empty): reads 0..8 share one reference of 900 bases that holds the
    calls of reads 0 and 2, the others have references of their own, the even ones around their own call"""
    rng = np.random.default_rng(31)
    lens = [int(x) for x in rng.integers(400, 3000, 18)]
    sigs = [_sig(n, 900 + i) for i, n in enumerate(lens)]
    calls = eng.basecall(sigs, "rnnrf_r94")

    def own(i):
        c = calls[i]
        return sa.encode_bases(c["bases"], 1).astype(np.int32) if c is not None and len(c["bases"]) >= 1 else np.zeros(0, dtype=np.int32)
    shared = np.concatenate((rng.integers(0, 4, 200), own(0), rng.integers(0, 4, 150), own(2), rng.integers(0, 4, 300))).astype(np.int32)
    codes = []
    for i in range(18):
        if i < 9:
            codes.append(shared)
        elif i % 2 == 0:
            codes.append(np.concatenate((rng.integers(0, 4, 10 * i), own(i), rng.integers(0, 4, 7))).astype(np.int32))
        else:
            codes.append(rng.integers(0, 4, 50 + 40 * i).astype(np.int32))
    return dict(sigs=sigs, codes=codes, lens=lens)


def _check_against_per_read(eng, sigs, codes, res, vit, path, skip=()):
    for i, (x, cd) in enumerate(zip(sigs, codes)):
        if i in skip:
            continue
        trans = eng.posterior(x, "rnnrf_r94")
        ws, wf, wl, wp = gpu_local(trans, cd, viterbi=vit, want=path)
        sc, first, last, pth = res[i]
        assert np.isfinite(ws) and _same_bits(sc, ws), (i, sc, ws)
        if vit:
            assert last == wl, i
        if vit and path:
            assert first == wf and len(pth) == trans.shape[0] + 1 and np.array_equal(pth, wp), i
            check_local_path(trans, cd, sc, first, last, pth)
        else:
            assert pth is None


def test_engine_map_local_batch(eng, call):
    res, rc, err = _batch(eng, call["sigs"], call["codes"])
    assert rc == 0, err
    _check_against_per_read(eng, call["sigs"], call["codes"], res, True, True)
    res, rc, err = _batch(eng, call["sigs"], call["codes"], vit=True, path=False)
    assert rc == 0, err
    _check_against_per_read(eng, call["sigs"], call["codes"], res, True, False)
    res, rc, err = _batch(eng, call["sigs"], call["codes"], vit=False, path=False)
    assert rc == 0, err
    _check_against_per_read(eng, call["sigs"], call["codes"], res, False, False)
    # the Python surface: strings, one for all reads or one per read
    refs = ["".join("ACGT"[b] for b in cd) for cd in call["codes"]]
    py = eng.map_to_reference(call["sigs"], refs, viterbi=True, path=True)
    want, _, _ = _batch(eng, call["sigs"], call["codes"])
    for (s, f, l, p), (ws, wf, wl, wp) in zip(py, want):
        assert _same_bits(s, ws) and (f, l) == (wf, wl) and np.array_equal(p, wp)
    one = eng.map_to_reference(call["sigs"][:9], refs[0], viterbi=True, path=True)
    for (s, f, l, p), (ws, wf, wl, wp) in zip(one, want[:9]):
        assert _same_bits(s, ws) and (f, l) == (wf, wl) and np.array_equal(p, wp)


def test_engine_several_launch_groups(eng, call):
    """the same call under a budget of 700 column blocks: at least three launch groups, the same bits"""
    uncut, rc, err = _batch(eng, call["sigs"], call["codes"])
    assert rc == 0, err
    form = (True, True, False)
    before = sa.map_crf_local_form_counts()[form]
    eng.set_max_launch_blocks(700)
    try:
        cut, rc, err = _batch(eng, call["sigs"], call["codes"])
    finally:
        eng.set_max_launch_blocks(0)
    assert rc == 0, err
    groups = (sa.map_crf_local_form_counts()[form] - before) // 2        # two passes per group
    print("launch groups under a budget of 700 blocks: %d" % groups)
    assert groups >= 3
    for i, (a, b) in enumerate(zip(uncut, cut)):
        assert _same_bits(a[0], b[0]) and a[1:3] == b[1:3] and np.array_equal(a[3], b[3]), i


def test_engine_scratch_windows(eng, call):
    """one window per sequence (the debug option at 0) on a reference longer than the LDS home: the tiled scratch forms"""
    rng = np.random.default_rng(43)
    ref = rng.integers(0, 4, max_cells() + 300).astype(np.int32)
    sigs, codes = call["sigs"][:3], [ref, ref, call["codes"][9]]
    want, rc, err = _batch(eng, sigs, codes)
    assert rc == 0, err
    eng.debug_option("map_crf_local_stride", 0)
    try:
        before = sa.map_crf_local_form_counts()
        res, rc, err = _batch(eng, sigs, codes)
        assert rc == 0, err
        fwd, rc2, err2 = _batch(eng, sigs, codes, vit=False, path=False)
        assert rc2 == 0, err2
        after = sa.map_crf_local_form_counts()
    finally:
        eng.debug_option("map_crf_local_stride", -1)
    assert after[(True, True, True)] - before[(True, True, True)] == 2 and after[(True, True, False)] - before[(True, True, False)] == 2
    assert after[(False, True, True)] - before[(False, True, True)] == 1 and after[(False, True, False)] - before[(False, True, False)] == 1
    for i, (a, b) in enumerate(zip(want, res)):
        assert _same_bits(a[0], b[0]) and a[1:3] == b[1:3] and np.array_equal(a[3], b[3]), i
    for i, (x, cd) in enumerate(zip(sigs, codes)):
        trans = eng.posterior(x, "rnnrf_r94")
        f64 = np_map_crf_local(trans, cd, viterbi=False, dtype=np.float64)[0]
        assert abs(float(fwd[i][0]) - float(f64)) <= 1e-4 * abs(float(f64)), i


def test_engine_refusals_leave_neighbours_untouched(eng, call):
    sigs = list(call["sigs"][:6])
    codes = list(call["codes"][:6])
    good, rc, err = _batch(eng, sigs, codes)
    assert rc == 0, err
    bad4 = codes[1].copy()
    bad4[17] = 4
    codes[1] = bad4                                        # a base code 4
    codes[3] = np.zeros(0, dtype=np.int32)                 # an empty sequence
    sigs[4] = _sig(5, 1)                                   # a read too short for the model
    res, rc, err = _batch(eng, sigs, codes)
    assert rc == 0 and "read 1" in err and "not a base" in err, err
    for i in (1, 3, 4):
        assert np.isnan(res[i][0]) and res[i][3] is None, i
    for i in (0, 2, 5):
        assert _same_bits(res[i][0], good[i][0]) and res[i][1:3] == good[i][1:3] and np.array_equal(res[i][3], good[i][3]), i
    res, rc, err = _batch(eng, sigs[3:5], codes[3:5])
    assert rc == 0 and "read 0" in err and "empty" in err, err
    res, rc, err = _batch(eng, sigs[4:5], codes[4:5])
    assert rc == 0 and "too short" in err, err
    py = eng.map_to_reference(sigs, ["".join("ACGT"[b] for b in cd if b < 4) if len(cd) else "" for cd in codes], viterbi=True, path=True)
    assert np.isnan(py[3][0]) and py[3][1:] == (None, None, None) and np.isnan(py[4][0]) and np.isfinite(py[0][0])


def test_transducer_model_is_refused(eng, call):
    with pytest.raises(RuntimeError, match="rgrgr_r94.*transducer"):
        eng.map_to_reference(call["sigs"][:2], "ACGTACGTAC", model="rgrgr_r94")
    assert "map_local_batch" in sa.last_error()


def test_seqmappy_inside_cli(eng, weights, tmp_path):
    """`scrappie seqmappy --model rnnrf_r94 --inside` on a bundled read and a FASTA that holds its call between flanks: the
    engine's result; the error cases; without the option a global run prints what it printed before"""
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    ds, dp = ref_decode_crf(eng.posterior(x, "rnnrf_r94"))
    seq, dpath = call_of(dp)
    assert len(seq) >= 1
    rng = np.random.default_rng(8)
    bases = "".join("ACGT"[b] for b in seq)
    ref = "".join(rng.choice(list("ACGT"), 1234)) + bases + "".join(rng.choice(list("ACGT"), 4321))
    fa, own = str(tmp_path / "ref.fa"), str(tmp_path / "own_call.fa")
    with open(fa, "w") as fh:
        fh.write(">ref\n%s\n" % ref)
    with open(own, "w") as fh:
        fh.write(">own_call\n%s\n" % bases)
    crf_file, tr_file = str(tmp_path / "rnnrf_r94.scrm"), str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(weights[0], crf_file)
    model.save_model(weights[1], tr_file)
    (score, first, last, path), = eng.map_to_reference([x], ref, viterbi=True, path=True)
    nblock = eng.read_blocks("rnnrf_r94", len(x))
    assert _same_bits(score, ds) and (first, last) == (ref.find(bases), ref.find(bases) + len(bases)) and np.array_equal(path, dpath + first)

    def text(f, score, path, nblock, tail=""):
        t = "# %s to %s -- score %f over %d blocks (%f per block)%s\nblock\tpos\n" % (f5, f, -score, nblock, np.float32(-score) / np.float32(nblock), tail)
        return t + "".join("%d\t%d\n" % (i, p) for i, p in enumerate(path))

    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--local", "4.0", "--inside", fa, f5],
                       capture_output=True, text=True, timeout=120)              # (--local is still --localpen)
    assert r.returncode == 0, r.stderr
    assert r.stdout == text(fa, np.float32(score), path, nblock, " bases %d..%d" % (first, last))
    assert len(r.stdout.splitlines()) == nblock + 3
    # without the option: the global run of before
    (gscore, gpath), = eng.map_to_sequence([x], [bases], model="rnnrf_r94", viterbi=True, path=True)
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, own, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == text(own, np.float32(gscore), gpath, nblock)
    # the error cases name the option
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--inside", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--inside" in r.stderr and r.stdout == ""
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--inside", "--all-records", fa, f5],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--inside" in r.stderr and "--all-records" in r.stderr and r.stdout == ""
    u = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    assert "--inside" in u.stderr + u.stdout


def test_every_map_crf_local_form_was_launched(forms_at_start, worst):
    """the last test of the module: each of the 8 k_map_crf_local instantiations (Viterbi / forward x reference layout / tiled x
    LDS / scratch) has been launched by the tests above"""
    now = sa.map_crf_local_form_counts()
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("k_map_crf_local launches by (viterbi, tiled, scratch): %r" % sorted(ran.items()))
    print("forward: worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f in LDS, %.3f in scratch" % (worst["lds"], worst["scratch"]))
    assert len(ran) == 8 and all(v > 0 for v in ran.values()), ran
