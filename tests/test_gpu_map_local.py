"""Reads of a transducer model mapped INTO a longer sequence of k-mer states on the GPU (k_map_local, sh_map_local.h): the per-read
symbols against the numpy restatement of tests/test_map_local_cpu.py at every stride and in both homes;
scrappie_hip_map_post_local_batch / Engine.map_to_reference_transducer against the per-read symbols on the read's own posterior;
`scrappie seqmappy --within`.  Viterbi scores, first, last and paths are bit-identical (where the one-window restatement met a
tie on its way: the restatement at the same cut); forward scores lie within |gpu - f64| <= 2 |np32 - f64| + 1e-5 |f64|, the
float32 restatement making the same cut and the same order of reduction."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_gpu_map_crf import READ, READS, _ip, _prepared, _same_bits
from test_map_local_cpu import NR3, PENS, check_local_path, max_cells, np_map_local, rand_post

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
NBLOCKS = (1, 2, 3, 65)
LENGTHS = (1, 2, 3, 255, 256, 257, 1000)         # around the workgroup's chunk of 256 cells
STRIDES = (1, 7, 64, -1, 0)
TR = "rgrgr_r94"


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """k_map_local launches per form before this module's first test (test_every_map_local_form_was_launched)"""
    return sa.map_local_form_counts()


@pytest.fixture(scope="module")
def worst():
    """the worst forward ratio |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) the module has seen, per home, printed by its last test"""
    return dict(lds=0.0, scratch=0.0)


@pytest.fixture(autouse=True)
def default_stride():
    yield
    sa.set_map_local_stride(-1)


class _PostMat(object):
    """a _Mat over a numpy [nblock][nr] log-posterior, columns whole 16-byte pieces apart as scrappie matrices are; the padding
    holds no probability"""

    def __init__(self, post):
        nb, nr = post.shape
        stride = (nr + 3) // 4 * 4
        self.buf = np.full((nb, stride), np.float32(777.0), dtype=np.float32)
        self.buf[:, :nr] = post
        self.mat = sa._Mat()
        self.mat.nr, self.mat.nrq, self.mat.nc, self.mat.stride = nr, stride // 4, nb, stride
        self.mat.data = self.buf.ctypes.data


def gpu_local(post, seq, pens=PENS[0], viterbi=True, stride=-1, want=True):
    """one per-read symbol at a stride of the window cut: (float32 score, first, last, path)"""
    L = sa.lib()
    sa.set_map_local_stride(stride)
    m = _PostMat(np.ascontiguousarray(post, dtype=np.float32))
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    if not viterbi:
        return np.float32(L.map_to_reference_forward(C.byref(m.mat), pens[0], pens[1], pens[2], _ip(seq), len(seq))), None, None, None
    path = np.full(post.shape[0], -7, dtype=np.int32)
    first, last = C.c_size_t(12345), C.c_size_t(12345)
    s = L.map_to_reference_viterbi(C.byref(m.mat), pens[0], pens[1], pens[2], _ip(seq), len(seq), C.byref(first) if want else None, C.byref(last),
                                   _ip(path) if want else None)
    return np.float32(s), (int(first.value) if want else None), int(last.value), (path if want else None)


def _forward_ok(got, np32, f64, worst, key):
    eg, er = abs(float(got) - float(f64)), abs(float(np32) - float(f64))
    print("forward (%s): gpu %.9g np32 %.9g f64 %.12g" % (key, got, np32, f64))
    assert eg <= 2 * er + 1e-5 * abs(float(f64)), (got, np32, f64)
    worst[key] = max(worst[key], eg / (2 * er + 1e-5 * abs(float(f64)) + 1e-30))


@pytest.fixture(scope="module")
def grid():
    """one k = 3 posterior per nblock and one sequence per L, computed once"""
    rng = np.random.default_rng(77)
    return dict(post={nb: rand_post(nb, NR3, rng) for nb in NBLOCKS}, seqs={L: rng.integers(0, NR3 - 1, L).astype(np.int32) for L in LENGTHS})


@pytest.mark.parametrize("nblock", NBLOCKS)
def test_viterbi_grid_against_restatement(nblock, grid):
    """score, first, last and path in bits at strides 1, 7, 64, the default and one window, under the four penalty sets"""
    post = grid["post"][nblock]
    n = free = 0
    for L in LENGTHS:
        seq = grid["seqs"][L]
        for pens in PENS:
            info = {}
            ws, wf, wl, wp = np_map_local(post, seq, *pens, info=info)
            check_local_path(post, seq, pens, ws, wf, wl, wp)
            n += 1
            free += info["tie_free"]
            for stride in STRIDES:
                gs, gf, gl, gp = gpu_local(post, seq, pens, stride=stride)
                assert _same_bits(gs, ws), (nblock, L, pens, stride, gs, ws)
                if not info["tie_free"]:                     # a tie on the way: the path is the same cut's
                    ws2, wf, wl, wp = np_map_local(post, seq, *pens, stride=stride)
                assert (gf, gl) == (wf, wl) and np.array_equal(gp, wp), (nblock, L, pens, stride, gf, gl, wf, wl)
            gs, gf, gl, gp = gpu_local(post, seq, pens, want=False)          # no path wanted: the first pass alone
            assert _same_bits(gs, ws) and gf is None and gp is None
            if info["tie_free"]:
                assert gl == wl
    print("tie-free: %d of %d (a read of one or two blocks meets its best k-mers again in a sequence of 1000)" % (free, n))


@pytest.mark.parametrize("nblock", NBLOCKS)
def test_forward_grid_against_restatement(nblock, grid, worst):
    post = grid["post"][nblock]
    for L in LENGTHS:
        seq = grid["seqs"][L]
        for pens in (PENS[0], PENS[1]) if L > 3 else PENS:
            f64 = np_map_local(post, seq, *pens, viterbi=False, dtype=np.float64)[0]
            for stride in STRIDES:
                if (stride == 1 and L * nblock > 1000) or (stride == 7 and L * nblock > 20000):
                    continue                                     # (the restatement walks the windows one by one)
                n32 = np_map_local(post, seq, *pens, stride=stride, viterbi=False)[0]
                _forward_ok(gpu_local(post, seq, pens, viterbi=False, stride=stride)[0], n32, f64, worst, "lds")


def test_lds_windows_and_one_scratch_window_agree(worst):
    """L = max_cells + 300, nblock = 40: the default stride (windows in LDS) and stride 0 (one window, in scratch)"""
    rng = np.random.default_rng(78)
    L = max_cells(NR3) + 300
    post, seq = rand_post(40, NR3, rng), rng.integers(0, NR3 - 1, L).astype(np.int32)
    assert sa.map_local_max_cells(NR3) == max_cells(NR3)
    assert not sa.map_local_plan(L, 40, NR3, -1)["home"].any() and sa.map_local_plan(L, 40, NR3, 0)["home"].tolist() == [1]
    one = np_map_local(post, seq)[0]
    f64 = np_map_local(post, seq, viterbi=False, dtype=np.float64)[0]
    for stride, scr in ((-1, False), (0, True)):
        ws, wf, wl, wp = np_map_local(post, seq, stride=stride)      # the path at the same cut: right whether or not there is a tie on it
        assert _same_bits(ws, one)
        check_local_path(post, seq, PENS[0], ws, wf, wl, wp)
        before = sa.map_local_form_counts()
        gs, gf, gl, gp = gpu_local(post, seq, stride=stride)
        after = sa.map_local_form_counts()
        assert after[(True, False, scr)] - before[(True, False, scr)] == 2 and after[(True, False, not scr)] == before[(True, False, not scr)]
        assert _same_bits(gs, ws) and (gf, gl) == (wf, wl) and np.array_equal(gp, wp), (stride, gs, ws)
        n32 = np_map_local(post, seq, stride=stride, viterbi=False)[0]
        _forward_ok(gpu_local(post, seq, viterbi=False, stride=stride)[0], n32, f64, worst, "scratch" if scr else "lds")
        assert sa.map_local_form_counts()[(False, False, scr)] == after[(False, False, scr)] + 1
    for pens in PENS[1:]:                                   # the scratch home under the other penalties
        ws = np_map_local(post, seq, *pens, stride=0)
        gs = gpu_local(post, seq, pens, stride=0)
        assert _same_bits(gs[0], ws[0]) and gs[1:3] == ws[1:3] and np.array_equal(gs[3], ws[3]), pens


def test_1025_state_posterior(worst):
    """nblock = 40 on a k = 5 posterior: the column of 257 pieces of 16 bytes, the last one holding the stay entry alone"""
    rng = np.random.default_rng(80)
    post, seq = rand_post(40, 1025, rng), rng.integers(0, 1024, 300).astype(np.int32)
    seq[:4] = (0, 1023, 1020, 3)                            # the column's first and last pieces
    one = np_map_local(post, seq)[0]
    f64 = np_map_local(post, seq, viterbi=False, dtype=np.float64)[0]
    for stride in (-1, 7, 0):
        ws, wf, wl, wp = np_map_local(post, seq, stride=stride)
        assert _same_bits(ws, one)
        check_local_path(post, seq, PENS[0], ws, wf, wl, wp)
        gs, gf, gl, gp = gpu_local(post, seq, stride=stride)
        assert _same_bits(gs, ws) and (gf, gl) == (wf, wl) and np.array_equal(gp, wp), (stride, gs, ws)
        n32 = np_map_local(post, seq, stride=stride, viterbi=False)[0]
        _forward_ok(gpu_local(post, seq, viterbi=False, stride=stride)[0], n32, f64, worst, "lds")


def test_refusals_per_read():
    L = sa.lib()
    m = _PostMat(np.zeros((4, NR3), dtype=np.float32))
    seq = np.array([0, 1, 2, 3, 0, 1, 2], dtype=np.int32)
    assert np.isnan(L.map_to_reference_viterbi(None, 0.0, 0.0, 4.0, _ip(seq), 7, None, None, None)) and "null" in sa.last_error()
    assert np.isnan(L.map_to_reference_forward(C.byref(m.mat), 0.0, 0.0, 4.0, None, 7)) and "null" in sa.last_error()
    assert np.isfinite(L.map_to_reference_viterbi(C.byref(m.mat), 0.0, 0.0, 4.0, _ip(seq), 7, None, None, None))
    for code in (NR3 - 1, -1):
        s2 = seq.copy()
        s2[5] = code
        assert np.isnan(L.map_to_reference_viterbi(C.byref(m.mat), 0.0, 0.0, 4.0, _ip(s2), 7, None, None, None)) and "k-mers" in sa.last_error()
    assert np.isnan(L.map_to_reference_forward(C.byref(m.mat), 0.0, 0.0, 4.0, _ip(seq), 0)) and "empty" in sa.last_error()
    bad = _PostMat(np.zeros((4, NR3), dtype=np.float32))
    bad.mat.stride = NR3
    assert np.isnan(L.map_to_reference_forward(C.byref(bad.mat), 0.0, 0.0, 4.0, _ip(seq), 7)) and "16-byte" in sa.last_error()


def test_scrappy_style_map_post_to_reference():
    rng = np.random.default_rng(3)
    post = rand_post(50, NR3, rng)
    bases = "".join(rng.choice(list("ACGT"), 120))
    codes = sa.encode_bases(bases, 3)
    ws, wf, wl, wp = np_map_local(post, codes, 0.5, 0.25, 3.0)
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    s, first, last, p = sa.map_post_to_reference(m, bases, 0.5, 0.25, 3.0, viterbi=True, path=True)
    assert _same_bits(s, ws) and (first, last) == (wf, wl) and np.array_equal(p, wp)
    s, first, last, p = sa.map_post_to_reference(m, bases, 0.5, 0.25, 3.0, viterbi=True)
    assert _same_bits(s, ws) and first is None and last == wl and p is None
    s, first, last, p = sa.map_post_to_reference(m, bases, 0.5, 0.25, 3.0)
    f64 = np_map_local(post, codes, 0.5, 0.25, 3.0, viterbi=False, dtype=np.float64)[0]
    assert p is None and abs(s - f64) < 1e-4 * abs(f64) and s >= ws


# ---------------------------------------------------------------------------
# the batched engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    return model.synthetic_model("rnnrf_r94", seed=11), model.synthetic_model(TR, seed=1)


@pytest.fixture(scope="module")
def eng(weights):
    e = sa.Engine(0)
    e.load_model("rnnrf_r94", weights[0])
    e.load_model(TR, weights[1])
    yield e
    e.close()


def _sig(n, seed):
    return synth.medmad_normalise(synth.synthetic_signal(n, seed))


EPENS = (0.5, 1.0, 4.0)


def _batch(eng, sigs, codes, vit=True, path=True, mdl=TR):
    """scrappie_hip_map_post_local_batch itself: codes[i] an int32 array (the same object for reads that share a sequence).
    Returns ([(score, first, last, path)], return code, error text)"""
    n = len(sigs)
    rts, keep = sa._raw_tables(sigs)
    tgs = (sa._MapLocalTarget * n)()
    for i, cd in enumerate(codes):
        tgs[i].seq = cd.ctypes.data_as(C.POINTER(C.c_int))
        tgs[i].seqlen = len(cd)
    out = (sa._MapLocalResult * n)()
    p = eng.default_params(min_prob=1e-5, tempW=1.0, tempb=1.0, stay_pen=EPENS[0], skip_pen=EPENS[1], local_pen=EPENS[2])
    rc = sa.lib().scrappie_hip_map_post_local_batch(eng._h, eng._models[mdl], rts, tgs, n, C.byref(p), 1 if vit else 0, 1 if path else 0, out)
    err = sa.last_error()
    res = []
    for r in (out[i] for i in range(n)):
        pth = np.ctypeslib.as_array(r.path, shape=(r.nblock,)).copy() if r.path else None
        res.append((np.float32(r.score), int(r.first), int(r.last), pth))
    sa.lib().scrappie_hip_free_map_local_results(out, n)
    return res, rc, err


@pytest.fixture(scope="module")
def call(eng):
    """18 reads of ragged lengths (two tiles, the second nearly empty): reads 0..8 share one reference that holds the calls of
    reads 0 and 2, the others have references of their own, the even ones around their own call"""
    rng = np.random.default_rng(31)
    lens = [int(x) for x in rng.integers(400, 3000, 18)]
    sigs = [_sig(n, 900 + i) for i, n in enumerate(lens)]
    calls = eng.basecall(sigs, TR)

    def rnd(n):
        return "".join(rng.choice(list("ACGT"), n))

    def own(i):
        c = calls[i]
        return c["bases"] if c is not None else ""
    shared = rnd(200) + own(0) + rnd(150) + own(2) + rnd(300)
    refs = [shared if i < 9 else (rnd(10 * i) + own(i) + rnd(7) if i % 2 == 0 else rnd(50 + 40 * i)) for i in range(18)]
    enc = {}
    codes = [enc.setdefault(r, np.ascontiguousarray(sa.encode_bases(r, 5), dtype=np.int32)) for r in refs]
    return dict(sigs=sigs, refs=refs, codes=codes, lens=lens, own=[own(i) for i in range(18)])


def _check_against_per_read(eng, sigs, codes, res, vit, path):
    for i, (x, cd) in enumerate(zip(sigs, codes)):
        post = eng.posterior(x, TR)
        ws, wf, wl, wp = gpu_local(post, cd, EPENS, viterbi=vit, want=path)
        sc, first, last, pth = res[i]
        assert np.isfinite(ws) and _same_bits(sc, ws), (i, sc, ws)
        if vit:
            assert last == wl, i
        if vit and path:
            assert first == wf and len(pth) == post.shape[0] and np.array_equal(pth, wp), i
            check_local_path(post, cd, EPENS, sc, first, last, pth)
        else:
            assert pth is None


def test_engine_map_post_local_batch(eng, call):
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
    kw = dict(model=TR, viterbi=True, path=True, stay_pen=EPENS[0], skip_pen=EPENS[1], local_pen=EPENS[2])
    py = eng.map_to_reference_transducer(call["sigs"], call["refs"], **kw)
    want, _, _ = _batch(eng, call["sigs"], call["codes"])
    for (s, f, l, p), (ws, wf, wl, wp) in zip(py, want):
        assert _same_bits(s, ws) and (f, l) == (wf, wl) and np.array_equal(p, wp)
    one = eng.map_to_reference_transducer(call["sigs"][:9], call["refs"][0], **kw)
    for (s, f, l, p), (ws, wf, wl, wp) in zip(one, want[:9]):
        assert _same_bits(s, ws) and (f, l) == (wf, wl) and np.array_equal(p, wp)
    t = eng.map_timing()
    print("map_timing: %r" % (t,))


def test_engine_local_is_never_below_global(eng, call):
    """the same pairs through Engine.map_to_sequence: the global paths are a subset"""
    idx = [i for i in range(18) if len(call["own"][i]) >= 5]
    assert len(idx) >= 12
    sigs, seqs = [call["sigs"][i] for i in idx], [call["own"][i] for i in idx]
    kw = dict(model=TR, viterbi=True, stay_pen=EPENS[0], skip_pen=EPENS[1], local_pen=EPENS[2])
    glob = eng.map_to_sequence(sigs, seqs, **kw)
    loc = eng.map_to_reference_transducer(sigs, seqs, **kw)
    for i, ((g, _), (s, f, l, p)) in enumerate(zip(glob, loc)):
        assert np.isfinite(g) and np.float32(s) >= np.float32(g), (i, s, g)


def test_engine_several_launch_groups(eng, call):
    """the same call under a budget of 700 column blocks: at least three launch groups, the same bits"""
    uncut, rc, err = _batch(eng, call["sigs"], call["codes"])
    assert rc == 0, err
    form = (True, True, False)
    before = sa.map_local_form_counts()[form]
    eng.set_max_launch_blocks(700)
    try:
        cut, rc, err = _batch(eng, call["sigs"], call["codes"])
    finally:
        eng.set_max_launch_blocks(0)
    assert rc == 0, err
    groups = (sa.map_local_form_counts()[form] - before) // 2        # two passes per group
    print("launch groups under a budget of 700 blocks: %d" % groups)
    assert groups >= 3
    for i, (a, b) in enumerate(zip(uncut, cut)):
        assert _same_bits(a[0], b[0]) and a[1:3] == b[1:3] and np.array_equal(a[3], b[3]), i


def test_engine_scratch_windows(eng, call):
    """one window per sequence (the debug option at 0) on a reference longer than the LDS home: the tiled scratch forms"""
    rng = np.random.default_rng(43)
    ref = rng.integers(0, 1024, max_cells(1025) + 300).astype(np.int32)
    sigs, codes = call["sigs"][:3], [ref, ref, call["codes"][9]]
    want, rc, err = _batch(eng, sigs, codes)
    assert rc == 0, err
    eng.debug_option("map_local_stride", 0)
    try:
        before = sa.map_local_form_counts()
        res, rc, err = _batch(eng, sigs, codes)
        assert rc == 0, err
        fwd, rc2, err2 = _batch(eng, sigs, codes, vit=False, path=False)
        assert rc2 == 0, err2
        after = sa.map_local_form_counts()
    finally:
        eng.debug_option("map_local_stride", -1)
    assert after[(True, True, True)] - before[(True, True, True)] == 2 and after[(True, True, False)] - before[(True, True, False)] == 2
    assert after[(False, True, True)] - before[(False, True, True)] == 1 and after[(False, True, False)] - before[(False, True, False)] == 1
    for i, (a, b) in enumerate(zip(want, res)):
        assert _same_bits(a[0], b[0]) and a[1:3] == b[1:3] and np.array_equal(a[3], b[3]), i
    dflt, rc, err = _batch(eng, sigs, codes, vit=False, path=False)
    assert rc == 0, err
    # the same paths summed in another order: each sum lies within 2 |np32 - f64| + 1e-5 |f64| of the float64 value by the per-read
    # rule above, and float32 loses about 1e-5 |f64| over these hundreds of blocks (the grid's printed figures): 1e-4 |f64| bounds the pair
    for i in range(3):
        assert abs(float(fwd[i][0]) - float(dflt[i][0])) <= 1e-4 * abs(float(dflt[i][0])), i


def test_engine_refusals_leave_neighbours_untouched(eng, call):
    sigs = list(call["sigs"][:6])
    codes = list(call["codes"][:6])
    good, rc, err = _batch(eng, sigs, codes)
    assert rc == 0, err
    bad = codes[1].copy()
    bad[17] = 1024
    codes[1] = bad                                         # the stay state is no k-mer
    codes[3] = np.zeros(0, dtype=np.int32)                 # an empty sequence
    sigs[4] = _sig(5, 1)                                   # a read too short for the model
    res, rc, err = _batch(eng, sigs, codes)
    assert rc == 0 and "read 1" in err and "k-mers" in err, err
    for i in (1, 3, 4):
        assert np.isnan(res[i][0]) and res[i][3] is None, i
    for i in (0, 2, 5):
        assert _same_bits(res[i][0], good[i][0]) and res[i][1:3] == good[i][1:3] and np.array_equal(res[i][3], good[i][3]), i
    res, rc, err = _batch(eng, sigs[3:5], codes[3:5])
    assert rc == 0 and "read 0" in err and "empty" in err, err
    res, rc, err = _batch(eng, sigs[4:5], codes[4:5])
    assert rc == 0 and "too short" in err, err
    py = eng.map_to_reference_transducer(sigs, [call["refs"][0], "ACGTNACGTT", call["refs"][2], "ACG", call["refs"][4], call["refs"][5]], viterbi=True, path=True)
    assert np.isnan(py[1][0]) and np.isnan(py[3][0]) and py[3][1:] == (None, None, None) and np.isnan(py[4][0]) and np.isfinite(py[0][0])


def test_crf_model_is_refused(eng, call):
    res, rc, err = _batch(eng, call["sigs"][:2], call["codes"][:2], mdl="rnnrf_r94")
    assert rc == -1 and "rnnrf_r94" in err and "flip-flop" in err and "map_local_batch" in err, err
    assert all(np.isnan(r[0]) and r[3] is None for r in res)
    with pytest.raises(RuntimeError, match="rnnrf_r94.*flip-flop"):
        eng.map_to_reference_transducer(call["sigs"][:2], "ACGTACGTAC", model="rnnrf_r94")
    with pytest.raises(RuntimeError, match="rgrgr_r94.*transducer"):      # and the flip-flop call goes on refusing the transducer models
        eng.map_to_reference(call["sigs"][:2], "ACGTACGTAC", model=TR)


def test_seqmappy_within_cli(eng, weights, tmp_path):
    """`scrappie seqmappy --within` on a bundled read and a FASTA that holds its call between flanks: the engine's result; the
    error cases name the option; without the option a global run prints what it printed before"""
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    rng = np.random.default_rng(8)
    bases = "".join(rng.choice(list("ACGT"), 60))            # (synthetic weights call next to nothing: any sequence serves)
    ref = "".join(rng.choice(list("ACGT"), 1234)) + bases + "".join(rng.choice(list("ACGT"), 4321))
    fa, own = str(tmp_path / "ref.fa"), str(tmp_path / "own_call.fa")
    with open(fa, "w") as fh:
        fh.write(">ref\n%s\n" % ref)
    with open(own, "w") as fh:
        fh.write(">own_call\n%s\n" % bases)
    crf_file, tr_file = str(tmp_path / "rnnrf_r94.scrm"), str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(weights[0], crf_file)
    model.save_model(weights[1], tr_file)
    (score, first, last, path), = eng.map_to_reference_transducer([x], ref, model=TR, viterbi=True, path=True)
    nblock = eng.read_blocks(TR, len(x))
    assert len(path) == nblock and 0 <= first < last <= len(ref) - 4
    check_local_path(eng.posterior(x, TR), sa.encode_bases(ref, 5), (0.0, 0.0, 4.0), score, first, last, path)

    def text(f, score, path, nblock, tail=""):
        t = "# %s to %s -- score %f over %d blocks (%f per block)%s\nblock\tpos\n" % (f5, f, -score, nblock, np.float32(-score) / np.float32(nblock), tail)
        return t + "".join("%d\t%d\n" % (i, p) for i, p in enumerate(path))

    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--within", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == text(fa, np.float32(score), path, nblock, " states %d..%d" % (first, last))
    assert len(r.stdout.splitlines()) == nblock + 2
    # without the option: the global run of before
    (gscore, gpath), = eng.map_to_sequence([x], [bases], model=TR, viterbi=True, path=True)
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, own, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == text(own, np.float32(gscore), gpath, nblock)
    # the error cases name the option
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--within", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--within" in r.stderr and r.stdout == ""
    for other in ("--all-records", "--inside", "--find"):
        r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--within", other, fa, f5], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--within" in r.stderr and other in r.stderr and r.stdout == "", other
    u = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    assert "--within" in u.stderr + u.stdout


def test_every_map_local_form_was_launched(forms_at_start, worst):
    """the last test of the module: each of the 8 k_map_local instantiations (Viterbi / forward x dense / tiled x LDS / scratch)
    has been launched by the tests above"""
    now = sa.map_local_form_counts()
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("k_map_local launches by (viterbi, tiled, scratch): %r" % sorted(ran.items()))
    print("forward: worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f in LDS, %.3f in scratch" % (worst["lds"], worst["scratch"]))
    assert len(ran) == 8 and all(v > 0 for v in ran.values()), ran
