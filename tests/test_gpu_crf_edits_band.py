"""The banded forms of k_crf_edits_rows and k_crf_edits on the device (csrc/sh_crf_edits.h): the per-read symbol map_crf_edits_banded
against the float32 restatement np_crf_edits_banded -- Viterbi in bits for base, sub, del, ins and the NaN pattern; forward within
the standing bound 2 |np32 - f64| + 1e-5 |f64| -- over block counts, sequences a wave and a chunk of threads long from both sides,
bands from the Viterbi path and along the diagonal, a band wider than a chunk of threads, a band whose low edge crosses 64 and 256
cells in mid-read and a band that lets nothing through; the full band against map_crf_edits in bits; base against
map_crf_to_sequence_*_banded in bits; the batched engine against the per-read symbol in bits, cut by a budget, with a shared
sequence and with banded and unbanded targets mixed; refusals; Engine.score_edits' bands; the command line.  The last test requires
all twelve banded kernel forms to have been launched by this module and none to use scratch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_crf_edits_band_cpu import np_crf_edits_banded
from test_gpu_crf_edits import _sig, _str, flat, gpu_edits, same_bits
from test_gpu_map_crf import READ, READS, _HostMat, _ip, _prepared, _sp, gpu_map
from test_map_crf_cpu import _trans, call_of, no_path_band, np_bounds_sane, np_decode_crf, np_map_crf, path_bands

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
NBLOCKS = (1, 2, 3, 17, 64, 65)
CELLS = (63, 64, 65, 255, 256, 257, 513)
PATH_KINDS = ("around", "exact", "low-edge", "high-edge")


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """launches per banded form before this module's first test (test_every_banded_form_was_launched_and_none_uses_scratch)"""
    return sa.crf_edits_band_form_counts()


@pytest.fixture(scope="module")
def worst():
    """the worst forward ratio |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) the module has seen, printed by its last test"""
    return dict(per_read=0.0)


def gpu_edits_banded(trans, seq, low, high, viterbi=True, stride=28):
    """the per-read symbol: (base, sub, dele, ins, return code, error text)"""
    m = _HostMat(np.ascontiguousarray(trans, dtype=np.float32), stride)
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    lo, hi = (np.ascontiguousarray(b, dtype=np.uintp) for b in (low, high))
    L = len(seq)
    base = C.c_float(123.0)
    sub, dele, ins = (np.full(max(k, 1), 123.0, dtype=np.float32) for k in (4 * L, L, 4 * (L + 1)))
    fp = C.POINTER(C.c_float)
    rc = sa.lib().map_crf_edits_banded(C.byref(m.mat), _ip(seq), L, _sp(lo), _sp(hi), 1 if viterbi else 0, C.byref(base),
                                       sub.ctypes.data_as(fp), dele.ctypes.data_as(fp), ins.ctypes.data_as(fp))
    return np.float32(base.value), sub[:4 * L].reshape(L, 4), dele[:L], ins.reshape(L + 1, 4), rc, sa.last_error()


def bands_of(trans, seq, kinds=PATH_KINDS, diagonals=(1, 8)):
    """[(name, low, high)]: the kinds of path_bands around np_map_crf's own Viterbi path (where the sequence has one) and the diagonal
    bands, every one valid"""
    NB, L = trans.shape[0], len(seq)
    out = []
    path = np_map_crf(trans, seq)[1]
    if path is not None:
        out += [(k,) + tuple(path_bands(path, L, k)) for k in kinds]
    out += [("diagonal-%d" % h,) + tuple(sa.map_crf_diagonal_band(NB, L, h)) for h in diagonals]
    assert all(np_bounds_sane(lo, hi, NB, L) for _, lo, hi in out)
    return out


def check_against_restatement(trans, seq, lo, hi, worst, tag, stride=28):
    want = np_crf_edits_banded(trans, seq, lo, hi, viterbi=True)
    got = gpu_edits_banded(trans, seq, lo, hi, viterbi=True, stride=stride)
    assert got[4] == 0, got[5]
    for name, g, w in zip(("base", "sub", "del", "ins"), got[:4], want):
        assert same_bits(g, w), (tag, name, np.flatnonzero(np.ravel(np.asarray(g) != np.asarray(w)))[:8])
    assert same_bits(got[0], gpu_map(trans, seq, viterbi=True, bands=(lo, hi), stride=stride)[0]), (tag, got[0])      # k_map_crf in the same band
    f32 = flat(np_crf_edits_banded(trans, seq, lo, hi, viterbi=False))
    f64 = flat(np_crf_edits_banded(trans, seq, lo, hi, viterbi=False, dtype=np.float64))
    fw = gpu_edits_banded(trans, seq, lo, hi, viterbi=False, stride=stride)
    assert fw[4] == 0, fw[5]
    assert same_bits(fw[0], gpu_map(trans, seq, viterbi=False, bands=(lo, hi), stride=stride)[0]), (tag, fw[0])
    g = flat(fw[:4])
    assert np.array_equal(np.isnan(g), np.isnan(f64)), (tag, np.flatnonzero(np.isnan(g) != np.isnan(f64))[:8])
    ok = ~np.isnan(f64)
    bound = 2 * np.abs(f32[ok] - f64[ok]) + 1e-5 * np.abs(f64[ok])
    err = np.abs(g[ok] - f64[ok])
    ratio = float(np.max(err / (bound + 1e-30))) if err.size else 0.0
    print("%s: forward worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f over %d scores, %d NaN" % (tag, ratio, err.size, int(np.sum(~ok))))
    assert np.all(err <= bound), (tag, float(np.max(err - bound)))
    worst["per_read"] = max(worst["per_read"], ratio)


# ---------------------------------------------------------------------------
# the per-read symbol
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nblock", NBLOCKS)
def test_block_counts_against_restatement(nblock, worst):
    rng = np.random.default_rng(700 + nblock)
    trans = _trans(nblock, 2.0, rng)
    seqs = [rng.integers(0, 4, L) for L in sorted(set((1, max(1, nblock // 2), nblock, nblock + 1)))]
    own = call_of(np_decode_crf(trans)[1])[0]
    if len(own):
        seqs.append(own)
    for k, seq in enumerate(seqs):
        for bname, lo, hi in bands_of(trans, seq):
            check_against_restatement(trans, seq, lo, hi, worst, "n%d L%d %s" % (nblock, len(seq), bname), stride=25 if k == 0 else 28)


@pytest.mark.parametrize("cells", CELLS)
def test_a_wave_and_a_chunk_of_threads_from_both_sides(cells, worst):
    rng = np.random.default_rng(800 + cells)
    L = cells - 1
    trans = _trans(L + 1 + cells % 7 if cells < 200 else L + L // 3, 2.0, rng)
    seq = rng.integers(0, 4, L)
    for bname, lo, hi in bands_of(trans, seq):
        check_against_restatement(trans, seq, lo, hi, worst, "cells %d %s" % (cells, bname))


def test_a_band_wider_than_a_chunk_of_threads(worst):
    """513 cells in a band of 301: more than one cell per thread in k_crf_edits_rows, rows of 304 floats"""
    rng = np.random.default_rng(21)
    L = 512
    trans = _trans(L + L // 3, 2.0, rng)
    seq = rng.integers(0, 4, L)
    lo, hi = sa.map_crf_path_band(np_map_crf(trans, seq)[1], L, 150)
    assert int(np.max(hi.astype(np.int64) - lo.astype(np.int64))) == 301
    check_against_restatement(trans, seq, lo, hi, worst, "513 cells, 301 wide")


def test_a_low_edge_that_crosses_64_and_256_cells_in_mid_read(worst):
    """the cells of an entry are laid on the threads from the 64-cell group of low[t] on, and the positions of k_crf_edits in chunks
    of 256: a band whose low edge passes both boundaries while the read runs"""
    rng = np.random.default_rng(22)
    L = 300
    trans = _trans(400, 2.0, rng)
    seq = rng.integers(0, 4, L)
    lo, hi = sa.map_crf_path_band(np_map_crf(trans, seq)[1], L, 5)
    mid = lo[10:-10].astype(np.int64)
    assert mid.min() < 64 and mid.max() > 256 and np.any(mid == 64) and np.any(mid == 256)
    check_against_restatement(trans, seq, lo, hi, worst, "low edge across 64 and 256")


def test_a_band_that_lets_nothing_through(worst):
    """no_path_band: base and every edit NaN, as the restatement has them"""
    rng = np.random.default_rng(23)
    for NB, L in ((17, 12), (64, 40), (65, 66)):
        trans = _trans(NB, 2.0, rng)
        seq = rng.integers(0, 4, L)
        lo, hi = no_path_band(NB, L)
        assert np_bounds_sane(lo, hi, NB, L)
        check_against_restatement(trans, seq, lo, hi, worst, "no path n%d L%d" % (NB, L))
        base, sub, dele, ins, rc, err = gpu_edits_banded(trans, seq, lo, hi)
        assert rc == 0 and np.isnan(base) and np.all(np.isnan(sub)) and np.all(np.isnan(dele)) and np.all(np.isnan(ins))


def test_the_full_band_is_map_crf_edits_in_bits():
    rng = np.random.default_rng(24)
    for NB, L in ((1, 1), (3, 4), (17, 9), (65, 64), (300, 257), (700, 513)):
        trans = _trans(NB, 2.0, rng)
        seq = rng.integers(0, 4, L)
        lo, hi = np.zeros(NB + 1, dtype=np.uintp), np.full(NB + 1, L + 1, dtype=np.uintp)
        for vit in (True, False):
            a = gpu_edits(trans, seq, viterbi=vit)
            b = gpu_edits_banded(trans, seq, lo, hi, viterbi=vit)
            assert a[4] == 0 and b[4] == 0, (a[5], b[5])
            for name, x, y in zip(("base", "sub", "del", "ins"), a[:4], b[:4]):
                assert same_bits(x, y), (NB, L, vit, name)


def test_bad_bands_per_read():
    trans = _trans(30, 2.0, np.random.default_rng(2))
    seq = np.array([0, 1, 2, 3, 3, 1], dtype=np.int32)
    lo, hi = sa.map_crf_diagonal_band(30, 6, 2)
    bad = lo.copy()
    bad[0] = 1
    base, sub, dele, ins, rc, err = gpu_edits_banded(trans, seq, bad, hi)
    assert rc == 0 and "bands are not valid" in err and np.isnan(base) and np.all(np.isnan(sub)) and np.all(np.isnan(ins)), err
    lo2, hi2 = sa.map_crf_diagonal_band(29, 6, 2)                      # made for a read of another block count: one entry short
    base, sub, dele, ins, rc, err = gpu_edits_banded(trans, seq, np.append(lo2, 0), np.append(hi2, 0))
    assert rc == 0 and "bands are not valid" in err and np.isnan(base), err
    m = _HostMat(trans)
    fp = C.POINTER(C.c_float)
    b = C.c_float(1.0)
    assert sa.lib().map_crf_edits_banded(C.byref(m.mat), _ip(seq), 6, None, _sp(hi), 1, C.byref(b), None, None, None) == -1
    assert "null argument" in sa.last_error() and np.isnan(b.value)
    base, sub, dele, ins, rc, err = gpu_edits_banded(trans, [0, 4, 1], *sa.map_crf_diagonal_band(30, 3, 2))
    assert rc == 0 and "not a base" in err and np.isnan(base), err
    mat = sa.ScrappyMatrix.from_numpy(trans, sloika=False)
    want = np_crf_edits_banded(trans, seq, lo, hi)
    for got in (sa.map_trans_edits(mat, "ACGTTC", bands=(lo, hi)), sa.map_trans_edits(mat, "ACGTTC", bands=2)):
        for g, w in zip(got, want):
            assert same_bits(g, w)
    assert same_bits(got[0], sa.map_trans_to_sequence(mat, "ACGTTC", viterbi=True, bands=2)[0])


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


@pytest.fixture(scope="module")
def call(eng):
    """18 reads (two tiles, the second nearly empty): a long read between two short ones first, then 1000 .. 3000 samples; their
    transitions, calls and Viterbi paths from Engine.map_to_sequence, the band of half-width 6 around each path, and the per-read
    symbol's results in those bands, Viterbi and forward, computed once"""
    rng = np.random.default_rng(47)
    lens = [900, 3600, 1100] + [int(x) for x in rng.integers(1000, 3000, 15)]
    sigs = [_sig(n, 700 + i) for i, n in enumerate(lens)]
    trans = [eng.posterior(x, "rnnrf_r94") for x in sigs]
    calls = [call_of(np_decode_crf(t)[1])[0] for t in trans]
    assert all(len(c) >= 2 for c in calls)
    mapped = eng.map_to_sequence(sigs, [_str(c) for c in calls], model="rnnrf_r94", viterbi=True, path=True)
    bands = []
    for (score, path), c, t in zip(mapped, calls, trans):
        lo, hi = sa.map_crf_path_band(path, len(c), 6)
        assert np_bounds_sane(lo, hi, len(t), len(c))             # the claim of scrappie_hip_map_crf_path_band, for every path made here
        bands.append((lo, hi))
    mats = [sa.ScrappyMatrix.from_numpy(t, sloika=False) for t in trans]
    per_read = {vit: [sa.map_trans_edits(m, c, viterbi=vit, bands=b) for m, c, b in zip(mats, calls, bands)] for vit in (True, False)}
    return dict(sigs=sigs, lens=lens, trans=trans, calls=calls, mats=mats, bands=bands, per_read=per_read)


def _same_results(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def _planned_row_bytes(calls, bands):
    return sa.crf_edits_band_plan([len(c) for c in calls], bands)[3] * 4


@pytest.mark.parametrize("viterbi", [True, False])
def test_engine_path_bands(eng, call, viterbi):
    """bands from map_crf_path_band on map_to_sequence's paths: the per-read symbol's bits; the timing's row bytes are the planner's"""
    res = eng.score_edits(call["sigs"], call["calls"], viterbi=viterbi, bands=call["bands"])
    assert len(res) == len(call["sigs"])
    for i, (r, w) in enumerate(zip(res, call["per_read"][viterbi])):
        assert _same_results(r, w), i
        assert np.isfinite(r[0]) and np.any(np.isfinite(r[1])), i
    k = eng.crf_edits_timing()
    assert k["launches"] == 1 and k["edits_ms"] > 0 and k["rows_forward_ms"] > 0 and k["rows_backward_ms"] > 0
    banded = _planned_row_bytes(call["calls"], call["bands"])
    full = sum(sa.lib().scrappie_hip_crf_edits_row_bytes(len(c), len(t)) for c, t in zip(call["calls"], call["trans"]))
    print("row bytes of the call: %d in the bands, %d without" % (banded, full))
    assert k["row_bytes"] == banded and banded == sum(sa.crf_edits_band_row_bytes(*b) for b in call["bands"]) and banded < full
    if viterbi:                                             # the band holds the Viterbi path: base is decode_crf's score
        for i, r in enumerate(res):
            assert same_bits(r[0], np_decode_crf(call["trans"][i])[0]), i


def test_engine_diagonal_bands_and_none(eng, call):
    """bands=8: map_crf_diagonal_band per read; bands=None: exactly the unbanded call, and only unbanded forms are launched"""
    res = eng.score_edits(call["sigs"][:6], call["calls"][:6], viterbi=True, bands=8)
    for i in range(6):
        lo, hi = sa.map_crf_diagonal_band(len(call["trans"][i]), len(call["calls"][i]), 8)
        assert _same_results(res[i], sa.map_trans_edits(call["mats"][i], call["calls"][i], viterbi=True, bands=(lo, hi))), i
    band0, plain0 = sa.crf_edits_band_form_counts(), sa.crf_edits_form_counts()
    none = eng.score_edits(call["sigs"][:6], call["calls"][:6], viterbi=True, bands=None)
    band1, plain1 = sa.crf_edits_band_form_counts(), sa.crf_edits_form_counts()
    assert band1 == band0 and sum(plain1.values()) == sum(plain0.values()) + 3
    for i in range(6):
        assert _same_results(none[i], sa.map_trans_edits(call["mats"][i], call["calls"][i], viterbi=True)), i


def test_engine_launches_cut_by_a_small_budget(eng, call):
    """a budget of 512 KB of banded rows and results: several launches of the three banded kernels inside the launch group, identical
    bytes; the banded bytes are what is counted -- the same budget holds fewer reads of the unbanded call"""
    key = ("edits", False, True)
    before = sa.crf_edits_band_form_counts()[key]
    eng.debug_option("crf_edits_budget_kb", 512)
    try:
        cut = eng.score_edits(call["sigs"], call["calls"], viterbi=False, bands=call["bands"])
        launches = sa.crf_edits_band_form_counts()[key] - before
        assert eng.crf_edits_timing()["launches"] == launches
        assert eng.crf_edits_timing()["row_bytes"] == _planned_row_bytes(call["calls"], call["bands"])
        plain0 = sa.crf_edits_form_counts()[key]
        eng.score_edits(call["sigs"], call["calls"], viterbi=False)
        plain = sa.crf_edits_form_counts()[key] - plain0
    finally:
        eng.debug_option("crf_edits_budget_kb", 0)
    print("launches under a budget of 512 KB: %d banded, %d unbanded" % (launches, plain))
    assert 2 <= launches < plain
    for i, (r, w) in enumerate(zip(cut, call["per_read"][False])):
        assert _same_results(r, w), i


def test_engine_shared_sequence_and_per_read_bands(eng, call):
    seq = call["calls"][1][:60]
    sigs = call["sigs"][:6]
    bands = [sa.map_crf_diagonal_band(len(call["trans"][i]), 60, 3 + 2 * i) for i in range(6)]
    shared = eng.score_edits(sigs, _str(seq), viterbi=True, bands=bands)
    for i in range(6):
        want = sa.map_trans_edits(call["mats"][i], seq, viterbi=True, bands=bands[i])
        assert _same_results(shared[i], want), i
        assert shared[i][1].shape == (60, 4) and shared[i][3].shape == (61, 4)


def test_engine_banded_and_unbanded_targets_in_one_call(eng, call):
    """None for a read: the full band through the unbanded forms, in the same call as its banded neighbours"""
    n = 7
    bands = [call["bands"][i] if i % 2 == 0 else None for i in range(n)]
    bands[4] = 5                                            # and a diagonal band among them
    band0, plain0 = sa.crf_edits_band_form_counts(), sa.crf_edits_form_counts()
    res = eng.score_edits(call["sigs"][:n], call["calls"][:n], viterbi=False, bands=bands)
    band1, plain1 = sa.crf_edits_band_form_counts(), sa.crf_edits_form_counts()
    assert sum(band1.values()) == sum(band0.values()) + 3 and sum(plain1.values()) == sum(plain0.values()) + 3
    for i in range(n):
        b = bands[i]
        want = sa.map_trans_edits(call["mats"][i], call["calls"][i], viterbi=False, bands=b)
        assert _same_results(res[i], want), i
    k = eng.crf_edits_timing()
    assert k["launches"] == 2
    want_bytes = sum(sa.lib().scrappie_hip_crf_edits_row_bytes(len(call["calls"][i]), len(call["trans"][i])) for i in (1, 3, 5))
    want_bytes += sum(sa.crf_edits_band_row_bytes(*call["bands"][i]) for i in (0, 2, 6))
    want_bytes += sa.crf_edits_band_row_bytes(*sa.map_crf_diagonal_band(len(call["trans"][4]), len(call["calls"][4]), 5))
    assert k["row_bytes"] == want_bytes


def test_engine_bad_bands_leave_neighbours_untouched(eng, call):
    n = 6
    bands = [call["bands"][i] for i in range(n)]
    lo, hi = (b.copy() for b in bands[1])
    lo[len(lo) // 2] = hi[len(lo) // 2]                     # an empty entry
    bands[1] = (lo, hi)
    bands[3] = (bands[3][0], bands[3][1][:-1])              # high one entry short
    bands[4] = (np.append(bands[4][0], bands[4][0][-1]), np.append(bands[4][1], bands[4][1][-1]))       # one too many
    res = eng.score_edits(call["sigs"][:n], call["calls"][:n], viterbi=True, bands=bands)
    err = sa.last_error()
    assert "read 1" in err and "bands are not valid" in err, err
    for i in (1, 3, 4):
        assert np.isnan(res[i][0]) and np.all(np.isnan(res[i][1])) and np.all(np.isnan(res[i][2])) and np.all(np.isnan(res[i][3])), i
        assert res[i][1].shape == (len(call["calls"][i]), 4), i
    for i in (0, 2, 5):
        assert _same_results(res[i], call["per_read"][True][i]), i


def test_refusals(eng, call):
    with pytest.raises(RuntimeError, match="rgrgr_r94.*transducer"):
        eng.score_edits(call["sigs"][:2], "ACGTACGTAC", model="rgrgr_r94", bands=4)
    assert "map_crf_edits_banded_batch" in sa.last_error()
    # scrappie_hip_map_crf_edits_batch itself goes on refusing a target with a band, with the text it had
    res = sa._score_edits(eng, sa.lib().scrappie_hip_map_crf_edits_batch, "map_crf_edits_batch", call["sigs"][:3], call["calls"][:3], "rnnrf_r94", True,
                          bands=[None, call["bands"][1], None])
    assert "read 1" in sa.last_error() and "bands are not part of this call" in sa.last_error()
    assert np.isnan(res[1][0]) and np.all(np.isnan(res[1][1]))
    for i in (0, 2):
        assert _same_results(res[i], sa.map_trans_edits(call["mats"][i], call["calls"][i], viterbi=True)), i


# ---------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------
def test_seqmappy_edits_band_cli(eng, weights, tmp_path):
    """`scrappie seqmappy --model rnnrf_r94 --edits --band 8` on a bundled read and a piece of its own call: the table parses to what
    Engine.score_edits gives in the band of half-width 8 around map_to_sequence's path; `--edits` alone prints what it printed"""
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    seq = call_of(np_decode_crf(eng.posterior(x, "rnnrf_r94"))[1])[0][:300]
    assert len(seq) >= 2
    fa = str(tmp_path / "draft.fa")
    with open(fa, "w") as fh:
        fh.write(">draft\n%s\n" % _str(seq))
    crf_file = str(tmp_path / "rnnrf_r94.scrm")
    model.save_model(weights[0], crf_file)
    nblock = eng.read_blocks("rnnrf_r94", len(x))
    L = len(seq)
    ((score, path),) = eng.map_to_sequence([x], [_str(seq)], model="rnnrf_r94", viterbi=True, path=True)
    band = sa.map_crf_path_band(path, L, 8)

    def table(res):
        base, sub, dele, ins = res

        def f(v):
            d = np.float32(v) - np.float32(base)
            return "nan" if np.isnan(d) else "%f" % d
        want = "# %s to %s -- edits of %d bases, score %f over %d blocks\n" % (f5, fa, L, base, nblock)
        want += "pos\tbase\tdel\tsubA\tsubC\tsubG\tsubT\tinsA\tinsC\tinsG\tinsT\n"
        for i in range(L):
            want += "\t".join(["%d" % i, "ACGT"[seq[i]], f(dele[i])] + [f(v) for v in sub[i]] + [f(v) for v in ins[i]]) + "\n"
        return want + "\t".join(["%d" % L] + ["-"] * 6 + [f(v) for v in ins[L]]) + "\n"
    (banded,) = eng.score_edits([x], [seq], viterbi=True, bands=[band])
    (plain,) = eng.score_edits([x], [seq], viterbi=True)
    assert not _same_results(banded, plain)                 # (the band binds somewhere: the two tables are not one)
    cmd = [CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--edits"]
    r = subprocess.run(cmd + ["--band", "8", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == table(banded)
    r = subprocess.run(cmd + [fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == table(plain), r.stderr
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--band", "8", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--band" in r.stderr and "--edits" in r.stderr and r.stdout == ""
    r = subprocess.run(cmd + ["--band", "-3", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--band" in r.stderr and r.stdout == ""
    u = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    assert "--band" in u.stderr + u.stdout


def test_every_banded_form_was_launched_and_none_uses_scratch(forms_at_start, worst):
    """the last test of the module: each of the 8 banded k_crf_edits_rows instantiations (Viterbi / forward x reference layout / tiled x
    forward / backward rows) and of the 4 banded k_crf_edits ones has been launched by the tests above; the loaded kernels need no scratch"""
    now = sa.crf_edits_band_form_counts()
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("launches by banded form: %r" % sorted(ran.items()))
    print("forward: worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f per read" % worst["per_read"])
    assert len(ran) == 12 and all(v > 0 for v in ran.values()), ran
    scratch = sa.crf_edits_band_scratch()
    print("scratch bytes per lane by banded form: %r" % sorted(scratch.items()))
    assert len(scratch) == 12 and all(v == 0 for v in scratch.values()), scratch
