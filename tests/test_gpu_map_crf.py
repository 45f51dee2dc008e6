"""Reads of a flip-flop (CRF) model mapped to base sequences on the GPU (k_map_crf, sh_map_crf.h): the per-read symbols against the
numpy restatement of tests/test_map_crf_cpu.py and, on the cases made from a call, against the compiled reference's decode_crf
(oracle/_ref/libref_decode.so); Engine.map_to_sequence with a CRF model against the per-read symbols on the read's own transitions;
`scrappie seqmappy --model rnnrf_r94`.  Viterbi scores and paths are bit-identical, ties included; forward scores lie within
|gpu - f64| <= 2 |np32 - f64| + 1e-5 |f64|, the float32 restatement standing in for a reference that has no such function."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_map_crf_cpu import (bounds_sane, call_of, crf_lds_max_seq, map_crf_cases, map_crf_scratch_cases, no_path_band, np_map_crf,
                              path_bands, ref_decode_crf)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
READS = os.path.join(ROOT, "tests", "golden", "reads")
READ = "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand"
PM = C.POINTER(sa._Mat)
BAND_KINDS = ("around", "low-edge", "high-edge", "exact", "stall-slide")


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """k_map_crf launches per form before this module's first test (test_every_map_crf_form_was_launched)"""
    return sa.map_crf_form_counts()


@pytest.fixture(scope="module")
def worst():
    """the worst forward ratio |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) the module has seen, printed by its last test"""
    return dict(lds=0.0, scratch=0.0)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _sp(a):
    return a.ctypes.data_as(C.POINTER(C.c_size_t))


class _HostMat(object):
    """a _Mat over a numpy [nblock][25] array with a column stride of its own (28: the container's padding; 25: none)"""

    def __init__(self, trans, stride=28):
        nb = trans.shape[0]
        self.buf = np.full((nb, stride), np.float32(777.0), dtype=np.float32)       # the padding holds no transition
        self.buf[:, :25] = trans
        self.flat = self.buf.reshape(-1)[:(nb - 1) * stride + 25].copy()                # ends at the last column's 25th float
        self.mat = sa._Mat()
        self.mat.nr, self.mat.nrq, self.mat.nc, self.mat.stride = 25, (stride + 3) // 4, nb, stride
        self.mat.data = self.flat.ctypes.data


def gpu_map(trans, seq, viterbi=True, bands=None, stride=28):
    """one per-read symbol: (float32 score, path or None)"""
    L = sa.lib()
    m = _HostMat(np.ascontiguousarray(trans, dtype=np.float32), stride)
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    path = np.full(trans.shape[0] + 1, -7, dtype=np.int32)
    if bands is None:
        if viterbi:
            s = L.map_crf_to_sequence_viterbi(C.byref(m.mat), _ip(seq), len(seq), _ip(path))
        else:
            s = L.map_crf_to_sequence_forward(C.byref(m.mat), _ip(seq), len(seq))
    else:
        lo, hi = (np.ascontiguousarray(b, dtype=np.uintp) for b in bands)
        if viterbi:
            s = L.map_crf_to_sequence_viterbi_banded(C.byref(m.mat), _ip(seq), len(seq), _sp(lo), _sp(hi), _ip(path))
        else:
            s = L.map_crf_to_sequence_forward_banded(C.byref(m.mat), _ip(seq), len(seq), _sp(lo), _sp(hi))
    return np.float32(s), (path if viterbi and not np.isnan(s) else None)


def _same_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


def _forward_ok(got, np32, f64, worst, key):
    eg, er = abs(float(got) - float(f64)), abs(float(np32) - float(f64))
    print("forward: gpu %.9g np32 %.9g f64 %.12g" % (got, np32, f64))
    assert eg <= 2 * er + 1e-5 * abs(float(f64)), (got, np32, f64)
    worst[key] = max(worst[key], eg / (2 * er + 1e-5 * abs(float(f64)) + 1e-30))


def check_case(c, worst, key, kinds=BAND_KINDS):
    """one case through the four per-read symbols: unbanded, the full band, and bands made from its Viterbi path"""
    trans, seq, name = c["trans"], c["seq"], c["name"]
    nb, L = trans.shape[0], len(seq)
    ws, wp = np_map_crf(trans, seq)
    gs, gp = gpu_map(trans, seq)
    if np.isnan(ws):
        assert np.isnan(gs) and "no admissible path" in sa.last_error(), name
        assert np.isnan(gpu_map(trans, seq, viterbi=False)[0]), name
        return
    assert _same_bits(gs, ws), (name, gs, ws)
    assert np.array_equal(gp, wp), name
    if c["from_call"]:
        ds, dp = ref_decode_crf(trans)
        assert _same_bits(gs, ds) and np.array_equal(gp, call_of(dp)[1]), name
    f32, f64 = np_map_crf(trans, seq, viterbi=False)[0], np_map_crf(trans, seq, viterbi=False, dtype=np.float64)[0]
    _forward_ok(gpu_map(trans, seq, viterbi=False)[0], f32, f64, worst, key)
    full = (np.zeros(nb + 1, dtype=np.uintp), np.full(nb + 1, L + 1, dtype=np.uintp))
    for bname, bands in [("full", full)] + [(k, path_bands(wp, L, k)) for k in kinds]:
        assert bounds_sane(bands[0], bands[1], nb, L), (name, bname)
        bs, bp = gpu_map(trans, seq, bands=bands, stride=25 if bname == "around" else 28)
        assert _same_bits(bs, ws) and np.array_equal(bp, wp), (name, bname, bs, ws)           # a band that holds the path: the unbanded bits
        b32 = np_map_crf(trans, seq, viterbi=False, low=bands[0], high=bands[1])[0]
        b64 = f64 if bname == "full" else np_map_crf(trans, seq, viterbi=False, low=bands[0], high=bands[1], dtype=np.float64)[0]
        _forward_ok(gpu_map(trans, seq, viterbi=False, bands=bands)[0], b32, b64, worst, key)


def test_per_read_against_restatement_and_decode_crf(worst):
    assert ref_decode_crf(np.zeros((1, 25), np.float32)) is not None, "oracle/_ref/libref_decode.so is required (build() makes it and it travels with the tree)"
    cases = map_crf_cases()
    assert sum(c["from_call"] for c in cases) == 24
    for c in cases:
        check_case(c, worst, "lds")


@pytest.mark.parametrize("k", range(8))
def test_per_read_scratch_cases(k, worst):
    """sequences around the LDS home's last length: unbanded, the full band, and bands whose low edge and whose high edge is the
    true path"""
    M = crf_lds_max_seq()
    c = map_crf_scratch_cases()[k]
    before = sa.map_crf_form_counts()
    check_case(c, worst, "scratch" if len(c["seq"]) > M else "lds", kinds=("low-edge", "high-edge"))
    after = sa.map_crf_form_counts()
    scr = len(c["seq"]) > M
    for vit in (True, False):
        assert after[(vit, False, scr)] - before[(vit, False, scr)] == 4 and after[(vit, False, not scr)] == before[(vit, False, not scr)]


def test_bands_that_differ_from_the_unbanded_run(worst):
    """bands that hug some other path, or none: scores and paths are the restatement's, not the unbanded ones"""
    n_other = 0
    for c in map_crf_cases():
        trans, seq, name = c["trans"], c["seq"], c["name"]
        nb, L = trans.shape[0], len(seq)
        ws, wp = np_map_crf(trans, seq)
        if np.isnan(ws) or L < 2 or nb < 3:
            continue
        # another admissible path: bases as late as the read allows, then the band around it
        other = np.clip(np.arange(nb + 1) - (nb + 1 - L), -1, L - 1)
        for kind in ("around", "exact"):
            lo, hi = path_bands(other, L, kind)
            assert bounds_sane(lo, hi, nb, L), (name, kind)
            bs, bp = np_map_crf(trans, seq, low=lo, high=hi)
            gs, gp = gpu_map(trans, seq, bands=(lo, hi))
            assert _same_bits(gs, bs) and np.array_equal(gp, bp), (name, kind)
            n_other += not np.array_equal(bp, wp)
            b32 = np_map_crf(trans, seq, viterbi=False, low=lo, high=hi)[0]
            b64 = np_map_crf(trans, seq, viterbi=False, low=lo, high=hi, dtype=np.float64)[0]
            _forward_ok(gpu_map(trans, seq, viterbi=False, bands=(lo, hi))[0], b32, b64, worst, "lds")
        for h in (0, 3):         # the diagonal band: whatever it holds
            lo, hi = sa.map_crf_diagonal_band(nb, L, h)
            bs, bp = np_map_crf(trans, seq, low=lo, high=hi)
            gs, gp = gpu_map(trans, seq, bands=(lo, hi))
            if np.isnan(bs):
                assert np.isnan(gs), (name, h)
            else:
                assert _same_bits(gs, bs) and np.array_equal(gp, bp), (name, h)
        if L >= 9 and nb >= 4 and 3 * nb >= L - 2:
            lo, hi = no_path_band(nb, L)
            for vit in (True, False):
                gs, gp = gpu_map(trans, seq, viterbi=vit, bands=(lo, hi))
                assert np.isnan(gs) and gp is None and "no admissible path" in sa.last_error(), (name, vit)
    assert n_other >= 10


def test_only_path_in_a_band_of_width_one():
    c = {x["name"]: x for x in map_crf_cases()}["only-path"]
    n = len(c["seq"])
    lo = np.arange(n, dtype=np.uintp) + 1
    lo[0] = 0
    hi = np.arange(n, dtype=np.uintp) + 2
    ws, wp = np_map_crf(c["trans"], c["seq"], low=lo, high=hi)
    gs, gp = gpu_map(c["trans"], c["seq"], bands=(lo, hi))
    assert _same_bits(gs, ws) and np.array_equal(gp, wp) and np.array_equal(gp, np.arange(n))
    assert _same_bits(gs, np_map_crf(c["trans"], c["seq"])[0])


def test_refusals():
    L = sa.lib()
    tr = np.zeros((4, 25), dtype=np.float32)
    seq = np.array([0, 1, 2], dtype=np.int32)
    m = _HostMat(tr)
    path = np.zeros(5, dtype=np.int32)
    assert np.isnan(L.map_crf_to_sequence_viterbi(None, _ip(seq), 3, _ip(path))) and "null" in sa.last_error()
    assert np.isnan(L.map_crf_to_sequence_forward(C.byref(m.mat), None, 3)) and "null" in sa.last_error()
    lo, hi = np.zeros(5, dtype=np.uintp), np.full(5, 4, dtype=np.uintp)
    assert np.isnan(L.map_crf_to_sequence_viterbi_banded(C.byref(m.mat), _ip(seq), 3, None, _sp(hi), _ip(path))) and "null" in sa.last_error()
    assert np.isnan(L.map_crf_to_sequence_forward_banded(C.byref(m.mat), _ip(seq), 3, _sp(lo), None)) and "null" in sa.last_error()
    assert np.isfinite(L.map_crf_to_sequence_viterbi(C.byref(m.mat), _ip(seq), 3, None))            # no path wanted
    bad = _HostMat(tr)
    bad.mat.nr = 24
    assert np.isnan(L.map_crf_to_sequence_viterbi(C.byref(bad.mat), _ip(seq), 3, _ip(path))) and "25 rows" in sa.last_error()
    bad.mat.nr, bad.mat.nc = 25, 0
    assert np.isnan(L.map_crf_to_sequence_forward(C.byref(bad.mat), _ip(seq), 3)) and "25 rows" in sa.last_error()
    for code in (4, -1):
        s2 = np.array([0, code, 2], dtype=np.int32)
        assert np.isnan(L.map_crf_to_sequence_viterbi(C.byref(m.mat), _ip(s2), 3, _ip(path))) and "not a base" in sa.last_error()
    assert np.isnan(L.map_crf_to_sequence_forward(C.byref(m.mat), _ip(seq), 0)) and "empty" in sa.last_error()
    hi[4] = 3
    assert np.isnan(L.map_crf_to_sequence_viterbi_banded(C.byref(m.mat), _ip(seq), 3, _sp(lo), _sp(hi), _ip(path))) and "bands" in sa.last_error()
    long = np.zeros(6, dtype=np.int32)             # L = nblock + 2
    assert np.isnan(L.map_crf_to_sequence_viterbi(C.byref(m.mat), _ip(long), 6, None)) and "no admissible path" in sa.last_error()
    assert np.isfinite(L.map_crf_to_sequence_viterbi(C.byref(m.mat), _ip(long), 5, None))


def test_scrappy_style_map_trans_to_sequence():
    c = {x["name"]: x for x in map_crf_cases()}["call-s2-n200"]
    m = sa.ScrappyMatrix.from_numpy(c["trans"], sloika=False)
    bases = "".join("ACGT"[b] for b in c["seq"])
    s, p = sa.map_trans_to_sequence(m, bases, viterbi=True, path=True)
    assert _same_bits(s, c["dscore"]) and np.array_equal(p, c["dpath"])
    s, p = sa.map_trans_to_sequence(m, bases, viterbi=True, path=True, bands=path_bands(c["dpath"], len(bases), "around"))
    assert _same_bits(s, c["dscore"]) and np.array_equal(p, c["dpath"])
    lo, hi = sa.map_crf_diagonal_band(200, len(bases), 12)
    s, p = sa.map_trans_to_sequence(m, bases, viterbi=True, path=True, bands=12)
    ws, wp = np_map_crf(c["trans"], c["seq"], low=lo, high=hi)
    assert _same_bits(s, ws) and np.array_equal(p, wp)
    s, p = sa.map_trans_to_sequence(m, bases)
    assert p is None and abs(s - np_map_crf(c["trans"], c["seq"], viterbi=False, dtype=np.float64)[0]) < 1e-3 * abs(s)
    with pytest.raises(RuntimeError, match="no admissible path"):
        sa.map_trans_to_sequence(m, "A" * 202, viterbi=True)


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


def _bases(n, rng):
    return "".join(rng.choice(list("ACGT"), n))


def _codes(bases):
    return sa.encode_bases(bases, 1).astype(np.int32)


def _per_read(trans, bases, vit, band):
    """the per-read symbol on a read's own transitions: (score, path or None), NaN where it refuses"""
    return gpu_map(trans, _codes(bases), viterbi=vit, bands=band)


def _check_call(eng, sigs, seqs, bands, nan_at, vit=True):
    """Engine.map_to_sequence on the call against the per-read symbols, read by read; returns the results and the call's error text"""
    res = eng.map_to_sequence(sigs, seqs, model="rnnrf_r94", viterbi=vit, path=vit, bands=bands)
    err = sa.last_error()
    assert len(res) == len(sigs)
    for i, (x, sq) in enumerate(zip(sigs, seqs)):
        sc, pth = res[i]
        if i in nan_at:
            assert np.isnan(sc) and pth is None, i
            continue
        trans = eng.posterior(x, "rnnrf_r94")
        ws, wp = _per_read(trans, sq, vit, None if bands is None else bands[i])
        assert np.isfinite(ws) and _same_bits(sc, ws), (i, sc, ws)
        if vit:
            assert len(pth) == trans.shape[0] + 1 and np.array_equal(pth, wp), i
        else:
            assert pth is None
    return res, err


@pytest.fixture(scope="module")
def call(eng):
    """17 reads of ragged lengths (two tiles, the second nearly empty) and one too short; each even read against its own call, the
    others against a random sequence; read 4: a sequence longer than its entries (no admissible path); every third read banded"""
    rng = np.random.default_rng(31)
    lens = [int(x) for x in rng.integers(400, 3000, 18)]
    lens[9] = 5                                            # below the model's minimum
    sigs = [_sig(n, 900 + i) for i, n in enumerate(lens)]
    calls = eng.basecall(sigs, "rnnrf_r94")
    nblock = [eng.read_blocks("rnnrf_r94", n) for n in lens]
    seqs, own = [], []
    for i, c in enumerate(calls):
        if i != 9 and i % 2 == 0 and c is not None and len(c["bases"]) >= 1:
            seqs.append(c["bases"]); own.append(i)
        else:
            seqs.append(_bases(max(1, nblock[i] // 3), rng))
    seqs[4] = _bases(nblock[4] + 2, rng)
    own = [i for i in own if i != 4]
    bands = [None] * len(sigs)
    for i in range(0, len(sigs), 3):
        if nblock[i] > 0:
            bands[i] = sa.map_crf_diagonal_band(nblock[i], len(seqs[i]), 40)
    return dict(sigs=sigs, seqs=seqs, bands=bands, own=own, calls=calls, nblock=nblock, nan_at=(4, 9))


def test_engine_map_to_sequence_crf(eng, call):
    assert len(call["own"]) >= 5
    res, err = _check_call(eng, call["sigs"], call["seqs"], call["bands"], call["nan_at"])
    assert "read 4" in err and "no admissible path" in err, err
    _check_call(eng, call["sigs"], call["seqs"], call["bands"], call["nan_at"], vit=False)
    # mapping a read to the engine's own call of it: decode_crf's score on the read's transitions, and the call's path.  The call is
    # crfpath_to_basecall over nblock of the path's nblock + 1 entries (scrappy passes npos = nblock): where decode_crf's very last
    # entry is a base, the call lacks it -- such a read is held with that base put back, and scores no higher without it.
    unbanded = eng.map_to_sequence(call["sigs"], call["seqs"], model="rnnrf_r94", viterbi=True, path=True)
    whole, want = list(call["seqs"]), {}
    for i in call["own"]:
        ds, dp = ref_decode_crf(eng.posterior(call["sigs"][i], "rnnrf_r94"))
        seq, path = call_of(dp)
        whole[i] = "".join("ACGT"[b] for b in seq)
        want[i] = (ds, path)
        assert _same_bits(call["calls"][i]["score"], ds), i
        if whole[i] == call["seqs"][i]:
            assert _same_bits(unbanded[i][0], ds) and np.array_equal(unbanded[i][1], path), i
        else:
            assert dp[-1] != 4 and whole[i][:-1] == call["seqs"][i], i
            assert unbanded[i][0] <= ds, i
        if call["bands"][i] is not None:
            assert res[i][0] <= unbanded[i][0]
    again = eng.map_to_sequence(call["sigs"], whole, model="rnnrf_r94", viterbi=True, path=True)
    for i in call["own"]:
        assert _same_bits(again[i][0], want[i][0]) and np.array_equal(again[i][1], want[i][1]), i


def test_engine_crf_several_launch_groups(eng, call):
    """the same call under a budget of 700 column blocks: several launch groups, the same bits"""
    kw = dict(model="rnnrf_r94", viterbi=True, path=True, bands=call["bands"])
    uncut = eng.map_to_sequence(call["sigs"], call["seqs"], **kw)
    form = (True, True, False)
    before = sa.map_crf_form_counts()[form]
    eng.set_max_launch_blocks(700)
    try:
        cut = eng.map_to_sequence(call["sigs"], call["seqs"], **kw)
    finally:
        eng.set_max_launch_blocks(0)
    groups = sa.map_crf_form_counts()[form] - before
    print("launch groups under a budget of 700 blocks: %d" % groups)
    assert groups >= 3
    for i, ((a, pa), (b, pb)) in enumerate(zip(uncut, cut)):
        if i in call["nan_at"]:
            assert np.isnan(a) and np.isnan(b) and pa is None and pb is None
        else:
            assert _same_bits(a, b) and np.array_equal(pa, pb), i


def test_engine_crf_lds_and_scratch_in_one_group(eng):
    """a sequence longer than the LDS home takes beside short ones in one launch group: one launch of either home"""
    M = crf_lds_max_seq()
    rng = np.random.default_rng(41)
    lens = [900, 5 * (M + 40), 5 * (M + 40) + 7, 5 * (M + 700) + 3, 700]
    sigs = [_sig(n, 950 + i) for i, n in enumerate(lens)]
    nblock = [eng.read_blocks("rnnrf_r94", n) for n in lens]
    assert nblock[1] >= M + 8 and nblock[3] >= M + 600
    seqs = [_bases(nblock[0] // 2, rng), _bases(M + 1, rng), _bases(M, rng), _bases(M + 600, rng), _bases(50, rng)]
    bands = [None, None, None, sa.map_crf_diagonal_band(nblock[3], M + 600, 100), sa.map_crf_diagonal_band(nblock[4], 50, 10)]
    before = sa.map_crf_form_counts()
    _check_call(eng, sigs, seqs, bands, ())
    after = sa.map_crf_form_counts()
    assert after[(True, True, True)] - before[(True, True, True)] == 1 and after[(True, True, False)] - before[(True, True, False)] == 1
    before = after
    _check_call(eng, sigs, seqs, bands, (), vit=False)
    after = sa.map_crf_form_counts()
    assert after[(False, True, True)] - before[(False, True, True)] == 1 and after[(False, True, False)] - before[(False, True, False)] == 1


def test_transducer_calls_are_untouched(eng, call):
    """a transducer map_to_sequence call before and after a CRF call on the same engine: identical bytes"""
    rng = np.random.default_rng(51)
    sigs = call["sigs"][:8]
    seqs = [_bases(int(rng.integers(20, 200)), rng) for _ in sigs]
    kw = dict(model="rgrgr_r94", viterbi=True, path=True, stay_pen=0.5, skip_pen=1.0, local_pen=4.0)
    first = eng.map_to_sequence(sigs, seqs, **kw)
    fb = eng.map_to_sequence(sigs, seqs, bands=4, **dict(kw, path=False))
    eng.map_to_sequence(call["sigs"], call["seqs"], model="rnnrf_r94", viterbi=True, path=True, bands=call["bands"])
    again = eng.map_to_sequence(sigs, seqs, **kw)
    ab = eng.map_to_sequence(sigs, seqs, bands=4, **dict(kw, path=False))
    assert any(np.isfinite(s) for s, _ in first)
    for (a, pa), (b, pb) in zip(first + fb, again + ab):
        assert np.float32(a).tobytes() == np.float32(b).tobytes()
        assert (pa is None and pb is None) or pa.tobytes() == pb.tobytes()


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


def test_seqmappy_cli(eng, weights, tmp_path):
    """`scrappie seqmappy --model rnnrf_r94` on a bundled read and the FASTA of its own call: nblock + 1 records, the Python path;
    with rgrgr_r94 on the same read: what Engine.map_to_sequence gives, as ever"""
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    ds, dp = ref_decode_crf(eng.posterior(x, "rnnrf_r94"))
    bases = "".join("ACGT"[b] for b in call_of(dp)[0])      # decode_crf's call, the base of its last entry included
    assert len(bases) >= 1 and bases.startswith(eng.basecall([x], "rnnrf_r94")[0]["bases"])
    fa = str(tmp_path / "own_call.fa")
    with open(fa, "w") as fh:
        fh.write(">own_call\n%s\n" % bases)
    crf_file, tr_file = str(tmp_path / "rnnrf_r94.scrm"), str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(weights[0], crf_file)
    model.save_model(weights[1], tr_file)

    def text(score, path, nblock):
        t = "# %s to %s -- score %f over %d blocks (%f per block)\nblock\tpos\n" % (f5, fa, -score, nblock, np.float32(-score) / np.float32(nblock))
        return t + "".join("%d\t%d\n" % (i, p) for i, p in enumerate(path))

    (score, path), = eng.map_to_sequence([x], [bases], model="rnnrf_r94", viterbi=True, path=True)
    nblock = eng.read_blocks("rnnrf_r94", len(x))
    assert len(path) == nblock + 1
    assert _same_bits(score, ds) and np.array_equal(path, call_of(dp)[1])
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == text(np.float32(score), path, nblock)
    assert len(r.stdout.splitlines()) == nblock + 3

    (score, path), = eng.map_to_sequence([x], [bases], model="rgrgr_r94", viterbi=True, path=True, stay_pen=0.0, skip_pen=0.0, local_pen=4.0,
                                         min_prob=1e-5)
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, fa, f5], capture_output=True, text=True, timeout=120)
    if path is None:                                       # a call shorter than a k-mer: both refuse
        assert r.returncode != 0
    else:
        assert r.returncode == 0, r.stderr
        assert r.stdout == text(np.float32(score), path, len(path))
    u = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    assert "rnnrf_r94" in u.stderr + u.stdout and "blocks + 1" in u.stderr + u.stdout


def test_every_map_crf_form_was_launched(forms_at_start, worst):
    """the last test of the module: each of the 8 k_map_crf instantiations (Viterbi / forward x reference layout / tiled x LDS /
    scratch) has been launched by the tests above"""
    now = sa.map_crf_form_counts()
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("k_map_crf launches by (viterbi, tiled, scratch): %r" % sorted(ran.items()))
    print("forward: worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f in LDS, %.3f in scratch" % (worst["lds"], worst["scratch"]))
    assert len(ran) == 8 and all(v > 0 for v in ran.values()), ran
