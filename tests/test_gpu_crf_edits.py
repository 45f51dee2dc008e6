"""k_crf_edits_rows and k_crf_edits on the device (csrc/sh_crf_edits.h): the per-read symbol map_crf_edits against the float32
restatement np_crf_edits -- Viterbi in bits for base, sub, del, ins and the NaN pattern; forward within the standing bound
2 |np32 - f64| + 1e-5 |f64| -- over block counts, sequences a wave and a chunk of threads long from both sides, the hand-made
cases and the LDS limit; the batched engine against the per-read symbol on the same transitions in bits; the highest edits
scored again by map_trans_to_sequences; the command line.  The last test requires all twelve kernel forms to have been launched
by this module."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_crf_edits_cpu import CASES, all_edits, np_crf_edits, pick
from test_gpu_map_crf import READ, READS, _HostMat, _prepared, gpu_map
from test_map_crf_cpu import _trans, call_of, crf_lds_max_seq, np_decode_crf, np_map_crf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
NBLOCKS = (1, 2, 3, 17, 64, 65)
CELLS = (63, 64, 65, 255, 256, 257, 513)


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """launches per form before this module's first test (test_every_crf_edits_form_was_launched)"""
    return sa.crf_edits_form_counts()


@pytest.fixture(scope="module")
def worst():
    """the worst forward ratio |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) the module has seen, printed by its last test"""
    return dict(per_read=0.0, cross=0.0)


def gpu_edits(trans, seq, viterbi=True, stride=28):
    """the per-read symbol: (base, sub, dele, ins, return code, error text)"""
    m = _HostMat(np.ascontiguousarray(trans, dtype=np.float32), stride)
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    L = len(seq)
    base = C.c_float(123.0)
    sub, dele, ins = (np.full(max(k, 1), 123.0, dtype=np.float32) for k in (4 * L, L, 4 * (L + 1)))
    fp = C.POINTER(C.c_float)
    rc = sa.lib().map_crf_edits(C.byref(m.mat), seq.ctypes.data_as(C.POINTER(C.c_int)), L, 1 if viterbi else 0, C.byref(base),
                                sub.ctypes.data_as(fp), dele.ctypes.data_as(fp), ins.ctypes.data_as(fp))
    return np.float32(base.value), sub[:4 * L].reshape(L, 4), dele[:L], ins.reshape(L + 1, 4), rc, sa.last_error()


def flat(res):
    """base and the 9 L + 4 edits of a result as one float64 array"""
    return np.concatenate([[res[0]], np.ravel(res[1]), np.ravel(res[2]), np.ravel(res[3])]).astype(np.float64)


def same_bits(a, b):
    """the same NaN pattern and, beside the NaNs, the same float32 bits"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def check_against_restatement(trans, seq, worst, tag, stride=28):
    want = np_crf_edits(trans, seq, viterbi=True)
    got = gpu_edits(trans, seq, viterbi=True, stride=stride)
    assert got[4] == 0, got[5]
    for name, g, w in zip(("base", "sub", "del", "ins"), got[:4], want):
        assert same_bits(g, w), (tag, name, np.flatnonzero(np.ravel(np.asarray(g) != np.asarray(w)))[:8])
    ws = np_map_crf(trans, seq)[0]
    assert same_bits(got[0], ws), (tag, got[0], ws)                      # k_map_crf's score of the sequence itself
    f32 = flat(np_crf_edits(trans, seq, viterbi=False))
    f64 = flat(np_crf_edits(trans, seq, viterbi=False, dtype=np.float64))
    fw = gpu_edits(trans, seq, viterbi=False, stride=stride)
    assert fw[4] == 0, fw[5]
    assert same_bits(fw[0], gpu_map(trans, seq, viterbi=False, stride=stride)[0]), (tag, fw[0])     # k_map_crf's forward score, bit for bit
    g = flat(fw[:4])
    assert np.array_equal(np.isnan(g), np.isnan(f64)), tag
    ok = ~np.isnan(f64)
    bound = 2 * np.abs(f32[ok] - f64[ok]) + 1e-5 * np.abs(f64[ok])
    err = np.abs(g[ok] - f64[ok])
    ratio = float(np.max(err / (bound + 1e-30))) if err.size else 0.0
    print("%s: forward worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f over %d scores" % (tag, ratio, err.size))
    assert np.all(err <= bound), (tag, float(np.max(err - bound)))
    worst["per_read"] = max(worst["per_read"], ratio)


# ---------------------------------------------------------------------------
# the per-read symbol
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nblock", NBLOCKS)
def test_block_counts_against_restatement(nblock, worst):
    rng = np.random.default_rng(300 + nblock)
    for sigma in (0.5, 3.0):
        trans = _trans(nblock, sigma, rng)
        seqs = [rng.integers(0, 4, L) for L in sorted(set((1, max(1, nblock // 2), nblock, nblock + 1)))]
        own = call_of(np_decode_crf(trans)[1])[0]
        if len(own):
            seqs.append(own)
        for k, seq in enumerate(seqs):
            check_against_restatement(trans, seq, worst, "n%d s%g L%d" % (nblock, sigma, len(seq)), stride=25 if k == 0 else 28)


@pytest.mark.parametrize("cells", CELLS)
def test_a_wave_and_a_chunk_of_threads_from_both_sides(cells, worst):
    rng = np.random.default_rng(400 + cells)
    L = cells - 1
    trans = _trans(L + 1 + cells % 7 if cells < 200 else L + L // 3, 2.0, rng)
    check_against_restatement(trans, rng.integers(0, 4, L), worst, "cells %d" % cells)


def test_hand_made_cases(worst):
    for name, trans, seq in CASES:
        if name.startswith("call-") and not name.endswith("n40"):
            continue
        check_against_restatement(trans, seq, worst, name)
    by = {n: (t, s) for n, t, s in CASES}
    base, sub, dele, ins, rc, err = gpu_edits(*by["only-path"])
    assert rc == 0 and np.isfinite(base) and np.all(np.isnan(ins)) and np.all(np.isfinite(sub))
    base, sub, dele, ins, rc, err = gpu_edits(*by["one-base"])
    assert rc == 0 and np.isnan(dele[0]) and np.all(np.isfinite(sub)) and np.all(np.isfinite(ins))
    base, sub, dele, ins, rc, err = gpu_edits(*by["all-zero"])
    assert base == 0 and np.all(sub == 0) and np.all(dele == 0) and np.all(ins == 0)


def test_the_longest_sequence_and_one_too_long():
    """scrappie_hip_map_crf_lds_max_seq() bases fill the LDS; one base more is refused with the text and everything is NaN"""
    M = crf_lds_max_seq()
    rng = np.random.default_rng(6)
    trans = _trans(M + 40, 2.0, rng)
    seq = rng.integers(0, 4, M + 1)
    want = np_crf_edits(trans, seq[:M])
    got = gpu_edits(trans, seq[:M])
    assert got[4] == 0, got[5]
    for g, w in zip(got[:4], want):
        assert same_bits(g, w)
    base, sub, dele, ins, rc, err = gpu_edits(trans, seq)
    assert rc == 0 and "too long for k_crf_edits" in err, err
    assert np.isnan(base) and np.all(np.isnan(sub)) and np.all(np.isnan(dele)) and np.all(np.isnan(ins))
    assert sub.shape == (M + 1, 4) and ins.shape == (M + 2, 4)


def test_bad_sequences_per_read():
    trans = _trans(30, 2.0, np.random.default_rng(2))
    base, sub, dele, ins, rc, err = gpu_edits(trans, [0, 4, 1])
    assert rc == 0 and "not a base" in err and np.isnan(base) and np.all(np.isnan(sub)) and np.all(np.isnan(ins)), err
    base, sub, dele, ins, rc, err = gpu_edits(trans, [])
    assert rc == 0 and "empty" in err and np.isnan(base) and np.all(np.isnan(ins)) and ins.shape == (1, 4), err
    m = sa.ScrappyMatrix.from_numpy(trans, sloika=False)
    want = np_crf_edits(trans, [0, 1, 2, 3, 3])
    got = sa.map_trans_edits(m, "ACGTT")
    assert got[1].shape == (5, 4) and got[2].shape == (5,) and got[3].shape == (6, 4)
    for g, w in zip(got, want):
        assert same_bits(g, w)
    assert same_bits(got[0], sa.map_trans_to_sequence(m, "ACGTT", viterbi=True)[0])
    assert np.isnan(sa.map_trans_edits(m, "ACGNT")[0]) and "empty" in sa.last_error()       # not bases: an empty sequence to the library


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
    """18 reads (two tiles, the second nearly empty): a long read between two short ones first, then 1000 .. 3000 samples; their
    transitions and calls, and the per-read symbol's results on them, Viterbi and forward, computed once"""
    rng = np.random.default_rng(43)
    lens = [900, 3600, 1100] + [int(x) for x in rng.integers(1000, 3000, 15)]
    sigs = [_sig(n, 900 + i) for i, n in enumerate(lens)]
    trans = [eng.posterior(x, "rnnrf_r94") for x in sigs]
    calls = [call_of(np_decode_crf(t)[1])[0] for t in trans]
    assert all(len(c) >= 2 for c in calls)
    mats = [sa.ScrappyMatrix.from_numpy(t, sloika=False) for t in trans]
    per_read = {vit: [sa.map_trans_edits(m, c, viterbi=vit) for m, c in zip(mats, calls)] for vit in (True, False)}
    return dict(sigs=sigs, lens=lens, trans=trans, calls=calls, mats=mats, per_read=per_read)


def _same_results(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("viterbi", [True, False])
def test_engine_per_read_sequences(eng, call, viterbi):
    res = eng.score_edits(call["sigs"], call["calls"], viterbi=viterbi)
    assert len(res) == len(call["sigs"])
    for i, (r, w) in enumerate(zip(res, call["per_read"][viterbi])):
        assert _same_results(r, w), i
        assert np.isfinite(r[0]) and np.any(np.isfinite(r[1])), i
    t = eng.map_timing()
    assert t["network_ms"] > 0 and t["map_ms"] > 0
    k = eng.crf_edits_timing()
    assert k["launches"] >= 1 and k["edits_ms"] > 0 and k["rows_forward_ms"] > 0 and k["rows_backward_ms"] > 0
    assert k["row_bytes"] == sum(sa.lib().scrappie_hip_crf_edits_row_bytes(len(c), len(t)) for c, t in zip(call["calls"], call["trans"]))
    if viterbi:                                             # the reads' own calls: base is decode_crf's score, no edit beats it by more than rounding
        for i, r in enumerate(res):
            ds = np_decode_crf(call["trans"][i])[0]
            assert same_bits(r[0], ds), i
            top = np.nanmax(flat(r)[1:])
            assert top <= float(ds) + 1e-5 * abs(float(ds)), (i, top, ds)


def test_engine_shared_sequence(eng, call):
    seq = call["calls"][1][:60]
    shared = eng.score_edits(call["sigs"][:6], _str(seq), viterbi=True)
    each = eng.score_edits(call["sigs"][:6], [seq.copy() for _ in range(6)], viterbi=True)
    codes = eng.score_edits(call["sigs"][:6], seq, viterbi=True)                 # an array of codes for all reads
    for i in range(6):
        want = sa.map_trans_edits(call["mats"][i], seq, viterbi=True)
        assert _same_results(shared[i], want) and _same_results(each[i], want) and _same_results(codes[i], want), i
        assert shared[i][1].shape == (60, 4) and shared[i][3].shape == (61, 4)


def test_engine_launches_cut_by_a_small_budget(eng, call):
    """a budget of 128 KB of rows and results: several launches of the three kernels inside the launch group, identical bytes; several
    launch groups under a budget of column blocks likewise"""
    key = ("edits", False, True)
    before = sa.crf_edits_form_counts()[key]
    eng.debug_option("crf_edits_budget_kb", 128)
    try:
        cut = eng.score_edits(call["sigs"], call["calls"], viterbi=False)
    finally:
        eng.debug_option("crf_edits_budget_kb", 0)
    launches = sa.crf_edits_form_counts()[key] - before
    assert eng.crf_edits_timing()["launches"] == launches
    print("launches under a budget of 128 KB: %d" % launches)
    assert launches >= 3
    for i, (r, w) in enumerate(zip(cut, call["per_read"][False])):
        assert _same_results(r, w), i
    before = sa.crf_edits_form_counts()[key]
    eng.set_max_launch_blocks(1500)
    try:
        cut = eng.score_edits(call["sigs"], call["calls"], viterbi=False)
    finally:
        eng.set_max_launch_blocks(0)
    groups = sa.crf_edits_form_counts()[key] - before
    print("launch groups under a budget of 1500 blocks: %d" % groups)
    assert groups >= 2
    for i, (r, w) in enumerate(zip(cut, call["per_read"][False])):
        assert _same_results(r, w), i


def test_engine_bad_targets_leave_neighbours_untouched(eng, call):
    sigs = list(call["sigs"][:7])
    seqs = [c.copy() for c in call["calls"][:7]]
    seqs[1] = seqs[1].copy()
    seqs[1][3] = 4                                          # not a base
    seqs[2] = np.zeros(0, dtype=np.int32)                   # empty
    seqs[3] = np.zeros(crf_lds_max_seq() + 1, dtype=np.int32)       # too long for k_crf_edits
    sigs[5] = _sig(5, 1)                                    # a read too short for the model
    res = eng.score_edits(sigs, seqs, viterbi=True)
    err = sa.last_error()
    assert "read 1" in err and "not a base" in err, err
    for i in (1, 2, 3, 5):
        assert np.isnan(res[i][0]) and np.all(np.isnan(res[i][1])) and np.all(np.isnan(res[i][2])) and np.all(np.isnan(res[i][3])), i
        assert res[i][1].shape == (len(seqs[i]), 4) and res[i][3].shape == (len(seqs[i]) + 1, 4), i
    for i in (0, 4, 6):
        assert _same_results(res[i], call["per_read"][True][i]), i
    eng.score_edits(sigs[3:4], seqs[3:4])
    assert "too long for k_crf_edits" in sa.last_error()
    eng.score_edits(sigs[5:6], seqs[5:6])
    assert "too short" in sa.last_error()


def test_transducer_model_is_refused(eng, call):
    with pytest.raises(RuntimeError, match="rgrgr_r94.*transducer"):
        eng.score_edits(call["sigs"][:2], "ACGTACGTAC", model="rgrgr_r94")
    assert "map_crf_edits_batch" in sa.last_error()


@pytest.mark.parametrize("viterbi", [True, False])
def test_the_highest_edits_scored_again_by_the_exact_engine(eng, call, worst, viterbi):
    """one read: the 20 highest edits by score_edits through map_trans_to_sequences, within 2 |np32 - f64| + 1e-5 |f64|"""
    i = 4
    trans, seq = call["trans"][i], call["calls"][i]
    (res,) = eng.score_edits([call["sigs"][i]], [seq], viterbi=viterbi)
    edits = all_edits(seq)
    sc = np.array([pick(res, *e) for e in edits], dtype=np.float64)
    order = [k for k in np.argsort(-np.where(np.isnan(sc), -np.inf, sc), kind="stable") if np.isfinite(sc[k])][:20]
    assert len(order) == 20
    edited = [sa.apply_edit(seq, *edits[k]) for k in order]
    again = sa.map_trans_to_sequences(call["mats"][i], edited, viterbi=viterbi)
    for k, ed, ag in zip(order, edited, again):
        f32 = float(np_map_crf(trans, ed, viterbi=viterbi, dtype=np.float32)[0])
        f64 = float(np_map_crf(trans, ed, viterbi=viterbi, dtype=np.float64)[0])
        bound = 2 * abs(f32 - f64) + 1e-5 * abs(f64)
        err = abs(sc[k] - float(ag))
        print("%s %r: edits %.9g exact %.9g f64 %.12g ratio %.3f" % ("viterbi" if viterbi else "forward", edits[k], sc[k], ag, f64, err / (bound + 1e-30)))
        assert err <= bound, (edits[k], sc[k], ag, f64)
        worst["cross"] = max(worst["cross"], err / (bound + 1e-30))


def test_seqmappy_edits_cli(eng, weights, tmp_path):
    """`scrappie seqmappy --model rnnrf_r94 --edits` on a bundled read and a piece of its own call: what Engine.score_edits gives;
    the refusals name the option and print nothing"""
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    seq = call_of(np_decode_crf(eng.posterior(x, "rnnrf_r94"))[1])[0][:300]       # a window of the call, as a polisher takes one
    assert len(seq) >= 2
    fa = str(tmp_path / "draft.fa")
    with open(fa, "w") as fh:
        fh.write(">draft\n%s\n" % _str(seq))
    crf_file, tr_file = str(tmp_path / "rnnrf_r94.scrm"), str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(weights[0], crf_file)
    model.save_model(weights[1], tr_file)
    ((base, sub, dele, ins),) = eng.score_edits([x], [seq], viterbi=True)
    nblock = eng.read_blocks("rnnrf_r94", len(x))
    L = len(seq)

    def f(v):
        d = np.float32(v) - np.float32(base)
        return "nan" if np.isnan(d) else "%f" % d
    want = "# %s to %s -- edits of %d bases, score %f over %d blocks\n" % (f5, fa, L, base, nblock)
    want += "pos\tbase\tdel\tsubA\tsubC\tsubG\tsubT\tinsA\tinsC\tinsG\tinsT\n"
    for i in range(L):
        want += "\t".join(["%d" % i, "ACGT"[seq[i]], f(dele[i])] + [f(v) for v in sub[i]] + [f(v) for v in ins[i]]) + "\n"
    want += "\t".join(["%d" % L] + ["-"] * 6 + [f(v) for v in ins[L]]) + "\n"
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--edits", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    # three pairs: a fasta that is not there, the good pair, a sequence too long -- the good pair's lines, and each failure under its own name and reason
    long_fa = str(tmp_path / "long.fa")
    with open(long_fa, "w") as fh:
        fh.write(">long\n%s\n" % ("ACGT" * (crf_lds_max_seq() // 4 + 1)))
    missing = str(tmp_path / "missing.fa")
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--edits", missing, f5, fa, f5, long_fa, f5],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout == want, r.stderr
    lines = r.stderr.splitlines()
    assert any("missing.fa" in ln for ln in lines) and not any("draft.fa" in ln for ln in lines), r.stderr
    assert [("too long for --edits" in ln) for ln in lines if "long.fa" in ln] == [True], r.stderr
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--edits", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--edits" in r.stderr and r.stdout == ""
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--edits", "--find", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--edits" in r.stderr and "--find" in r.stderr and r.stdout == ""
    u = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    assert "--edits" in u.stderr + u.stdout


def test_every_crf_edits_form_was_launched(forms_at_start, worst):
    """the last test of the module: each of the 8 k_crf_edits_rows instantiations (Viterbi / forward x reference layout / tiled x
    forward / backward rows) and of the 4 k_crf_edits ones has been launched by the tests above"""
    now = sa.crf_edits_form_counts()
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("launches by form: %r" % sorted(ran.items()))
    print("forward: worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f per read, %.3f on the edits scored again" % (worst["per_read"], worst["cross"]))
    assert len(ran) == 12 and all(v > 0 for v in ran.values()), ran
