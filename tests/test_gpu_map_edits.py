"""k_map_edits_rows and k_map_edits on the device (csrc/sh_map_edits.h): the per-read symbol map_post_edits on dense posteriors
against the float32 restatement np_map_edits -- Viterbi in bits for base, sub, del, ins and the NaN pattern; forward within the
standing bound 2 |np32 - f64| + 1e-5 |f64| -- at the position-chunk edges of k_map_edits, the staging and load-ahead depths and the
shortest sequences; the batched engine against the per-read symbol on the read's own posterior in bits, under every cut; the
highest edits scored again by map_post_to_sequences; the command line.  The last test requires all twelve kernel forms to have
been launched by this module."""
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_gpu_map_crf import READ, READS, _prepared
from test_map_cpu import np_map
from test_map_edits_cpu import PENS, all_edits, encode, make_post, np_map_edits, pick

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
TR = "rgrgr_r94"
STAGE, AHEAD = 4, 4                     # SH_ME_CH, SH_ME_D of csrc/sh_map_edits.h: blocks staged per barrier, blocks of rows in flight
# (name, k, L, NB): each named for the boundary where the kernels can go wrong
SHAPES = [("k2-L2-one-state", 2, 2, 7), ("k2-L3", 2, 3, 7), ("k2-L9", 2, 9, 21), ("k3-L12", 3, 12, 19),
          ("k5-L5-one-state", 5, 5, 9), ("k5-L6", 5, 6, 9), ("k5-L40", 5, 40, 66),
          ("k5-L255-chunk-minus-one", 5, 255, 170), ("k5-L256-chunk", 5, 256, 170), ("k5-L257-chunk-plus-one", 5, 257, 170),
          ("k5-L513-three-chunks", 5, 513, 300),
          ("k5-L5-one-block", 5, 5, 1), ("k5-one-block", 5, 9, 1), ("k5-stage-minus-one", 5, 9, STAGE - 1), ("k5-stage", 5, 9, STAGE), ("k5-stage-plus-one", 5, 9, STAGE + 1),
          ("k5-two-stages", 5, 9, 2 * STAGE), ("k5-two-stages-plus-one", 5, 9, 2 * STAGE + 1),
          ("k3-ahead-minus-one", 3, 7, AHEAD - 1), ("k3-ahead", 3, 7, AHEAD), ("k3-ahead-plus-one", 3, 7, AHEAD + 1)]


@pytest.fixture(scope="module", autouse=True)
def forms_at_start():
    """launches per form before this module's first test (test_every_map_edits_form_was_launched)"""
    return sa.map_edits_form_counts()


@pytest.fixture(scope="module")
def worst():
    """the worst forward ratio |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) the module has seen, printed by its last test"""
    return dict(per_read=0.0, cross=0.0)


def _str(codes):
    return "".join("ACGT"[b] for b in codes)


def flat(res):
    """the 9 L + 4 edits of a result as one float64 array"""
    return np.concatenate([np.ravel(res[1]), np.ravel(res[2]), np.ravel(res[3])]).astype(np.float64)


def same_bits(a, b):
    """the same NaN pattern and, beside the NaNs, the same float32 bits"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def check_against_restatement(post, seq, k, pens, worst, tag):
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    want = np_map_edits(post, seq, k, pens, viterbi=True)
    got = sa.map_post_edits(m, np.asarray(seq, dtype=np.int32), *pens, viterbi=True)
    for name, g, w in zip(("base", "sub", "del", "ins"), got, want):
        assert same_bits(g, w), (tag, name, np.flatnonzero(np.ravel(np.asarray(g)).view(np.int32) != np.ravel(np.asarray(w, dtype=np.float32)).view(np.int32))[:8])
    assert same_bits(got[0], sa.map_post_to_sequence(m, _str(seq), *pens, viterbi=True)[0]), tag      # k_map's score of the sequence itself
    f32 = flat(np_map_edits(post, seq, k, pens, viterbi=False))
    f64 = flat(np_map_edits(post, seq, k, pens, viterbi=False, dtype=np.float64))
    fw = sa.map_post_edits(m, np.asarray(seq, dtype=np.int32), *pens, viterbi=False)
    assert same_bits(fw[0], sa.map_post_to_sequence(m, _str(seq), *pens, viterbi=False)[0]), tag     # k_map's forward score, bit for bit
    g = flat(fw)
    assert np.array_equal(np.isnan(g), np.isnan(f64)), (tag, np.flatnonzero(np.isnan(g) != np.isnan(f64))[:8])
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
def test_the_smallest_case_first(worst):
    """k = 2, two bases, one state: the first launch of the three kernels"""
    rng = np.random.default_rng(1)
    check_against_restatement(make_post(7, 2, rng), rng.integers(0, 4, 2), 2, PENS[0], worst, "smallest")


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_against_restatement(shape, worst):
    name, k, L, NB = shape
    rng = np.random.default_rng(700 + 13 * L + NB)
    check_against_restatement(make_post(NB, k, rng), rng.integers(0, 4, L), k, PENS[(L + NB) % 2], worst, name)


def test_homopolymer_and_a_low_stay_row(worst):
    rng = np.random.default_rng(8)
    check_against_restatement(make_post(40, 5, rng), np.full(23, 3), 5, PENS[1], worst, "homopolymer")
    check_against_restatement(make_post(30, 3, rng, stay_low=True), rng.integers(0, 4, 14), 3, PENS[0], worst, "stay-low")


def test_bad_sequences_per_read():
    rng = np.random.default_rng(2)
    post = make_post(30, 3, rng)
    m = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    for seq, text in (([0, 4, 1, 2], "not a base"), ([], "empty"), ([0, 1], "shorter than the model's k-mer")):
        base, sub, dele, ins = sa.map_post_edits(m, np.asarray(seq, dtype=np.int32), viterbi=True)
        assert text in sa.last_error(), sa.last_error()
        assert np.isnan(base) and np.all(np.isnan(sub)) and np.all(np.isnan(dele)) and np.all(np.isnan(ins)) and ins.shape == (len(seq) + 1, 4)
    want = np_map_edits(post, [0, 1, 2, 3, 3], 3, PENS[0])
    got = sa.map_post_edits(m, "ACGTT")
    for g, w in zip(got, want):
        assert same_bits(g, w)
    M = sa.lib().scrappie_hip_map_edits_max_bases(3)
    base, sub, dele, ins = sa.map_post_edits(m, np.zeros(M + 1, dtype=np.int32))
    assert "too long for k_map_edits" in sa.last_error() and np.isnan(base) and sub.shape == (M + 1, 4) and np.all(np.isnan(sub))


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


def _codes(bases):
    return np.array(["ACGT".index(b) for b in bases], dtype=np.int32)


@pytest.fixture(scope="module")
def call(eng):
    """18 reads (two tiles, the second nearly empty): a long read between two short ones first, then 1000 .. 3000 samples; their
    posteriors and calls, and the per-read symbol's results on them, Viterbi and forward, computed once"""
    rng = np.random.default_rng(43)
    lens = [900, 3600, 1100] + [int(x) for x in rng.integers(1000, 3000, 15)]
    sigs = [_sig(n, 900 + i) for i, n in enumerate(lens)]
    posts = [eng.posterior(x, TR) for x in sigs]
    own = [_codes(c["bases"]) for c in eng.basecall(sigs, TR)]
    assert all(len(c) >= 5 for c in own)
    # the synthetic weights call a read in a single k-mer: beside its own call every read has a draft of a third of its blocks in bases
    calls = [rng.integers(0, 4, len(p) // 3).astype(np.int32) for p in posts]
    mats = [sa.ScrappyMatrix.from_numpy(p, sloika=False) for p in posts]
    per_read = {vit: [sa.map_post_edits(m, c, viterbi=vit) for m, c in zip(mats, calls)] for vit in (True, False)}
    per_read_own = {vit: [sa.map_post_edits(m, c, viterbi=vit) for m, c in zip(mats, own)] for vit in (True, False)}
    return dict(sigs=sigs, lens=lens, posts=posts, calls=calls, own=own, mats=mats, per_read=per_read, per_read_own=per_read_own)


def _same_results(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("which", ["own", "calls"])
@pytest.mark.parametrize("viterbi", [True, False])
def test_engine_per_read_sequences(eng, call, viterbi, which):
    """the tiled layout and fin_post: the engine on the resident posterior gives the bits of the per-read symbol on eng.posterior,
    each read against its own call and against its draft"""
    res = eng.score_edits_transducer(call["sigs"], call[which], viterbi=viterbi)
    assert len(res) == len(call["sigs"])
    for i, (r, w) in enumerate(zip(res, call["per_read_own" if which == "own" else "per_read"][viterbi])):
        assert _same_results(r, w), i
        assert np.isfinite(r[0]) and np.any(np.isfinite(r[1])), i
    t = eng.map_timing()
    assert t["network_ms"] > 0 and t["map_ms"] > 0
    k = eng.map_edits_timing()
    assert k["launches"] >= 1 and k["edits_ms"] > 0 and k["rows_forward_ms"] > 0 and k["rows_backward_ms"] > 0
    assert k["row_bytes"] == sum(sa.lib().scrappie_hip_map_edits_row_bytes(len(c), 5, len(p)) for c, p in zip(call[which], call["posts"]))
    mapped = eng.map_to_sequence(call["sigs"], [_str(c) for c in call[which]], viterbi=viterbi)
    for i, r in enumerate(res):
        assert same_bits(r[0], mapped[i][0]), i                       # base: k_map's score through the batched mapping engine


def test_engine_shared_sequence(eng, call):
    seq = call["calls"][1][:60]
    shared = eng.score_edits_transducer(call["sigs"][:6], _str(seq), viterbi=True)
    each = eng.score_edits_transducer(call["sigs"][:6], [seq.copy() for _ in range(6)], viterbi=True)
    codes = eng.score_edits_transducer(call["sigs"][:6], seq, viterbi=True)                 # an array of codes for all reads
    for i in range(6):
        want = sa.map_post_edits(call["mats"][i], seq, viterbi=True)
        assert _same_results(shared[i], want) and _same_results(each[i], want) and _same_results(codes[i], want), i
        assert shared[i][1].shape == (60, 4) and shared[i][3].shape == (61, 4)


def test_engine_penalties_reach_the_kernels(eng, call):
    (got,) = eng.score_edits_transducer(call["sigs"][2:3], [call["calls"][2]], viterbi=True, stay_pen=0.3, skip_pen=0.7, local_pen=2.0)
    want = sa.map_post_edits(call["mats"][2], call["calls"][2], 0.3, 0.7, 2.0, viterbi=True)
    assert _same_results(got, want) and not same_bits(got[1], call["per_read"][True][2][1])


def test_engine_launches_cut_by_a_small_budget(eng, call):
    """a budget of 128 KB of rows and results: several launches of the three kernels inside the launch group, identical bytes; several
    launch groups under a budget of column blocks likewise"""
    key = ("edits", False, True)
    before = sa.map_edits_form_counts()[key]
    eng.debug_option("map_edits_budget_kb", 128)
    try:
        cut = eng.score_edits_transducer(call["sigs"], call["calls"], viterbi=False)
    finally:
        eng.debug_option("map_edits_budget_kb", 0)
    launches = sa.map_edits_form_counts()[key] - before
    assert eng.map_edits_timing()["launches"] == launches
    print("launches under a budget of 128 KB: %d" % launches)
    assert launches >= 3
    for i, (r, w) in enumerate(zip(cut, call["per_read"][False])):
        assert _same_results(r, w), i
    # A transducer's launch group is priced at about 100 KB per column block (the posterior of 1025 states), so these 18 reads and
    # their drafts come to some 1250 blocks and 1500 do not cut them; against two bases per block -- every state reached by a skip --
    # the rows bring them to some 1670, and the cut falls inside the call
    long_seqs = [np.random.default_rng(70 + i).integers(0, 4, 2 * len(p)).astype(np.int32) for i, p in enumerate(call["posts"])]
    want = [sa.map_post_edits(m, c, viterbi=False) for m, c in zip(call["mats"], long_seqs)]
    before = sa.map_edits_form_counts()[key]
    eng.set_max_launch_blocks(1500)
    try:
        cut = eng.score_edits_transducer(call["sigs"], long_seqs, viterbi=False)
    finally:
        eng.set_max_launch_blocks(0)
    groups = sa.map_edits_form_counts()[key] - before
    print("launch groups under a budget of 1500 blocks: %d" % groups)
    assert groups >= 2
    for i, (r, w) in enumerate(zip(cut, want)):
        assert _same_results(r, w) and np.any(np.isfinite(r[1])), i


def test_engine_bad_targets_leave_neighbours_untouched(eng, call):
    sigs = list(call["sigs"][:8])
    seqs = [c.copy() for c in call["calls"][:8]]
    seqs[1][3] = 4                                          # not a base
    seqs[2] = np.zeros(0, dtype=np.int32)                   # empty
    seqs[3] = np.zeros(sa.lib().scrappie_hip_map_edits_max_bases(5) + 1, dtype=np.int32)       # one state too long for k_map_edits
    sigs[5] = _sig(5, 1)                                    # a read too short for the model
    seqs[7] = seqs[7][:4]                                   # k - 1 bases
    res = eng.score_edits_transducer(sigs, seqs, viterbi=True)
    err = sa.last_error()
    assert "read 1" in err and "not a base" in err, err
    for i in (1, 2, 3, 5, 7):
        assert np.isnan(res[i][0]) and np.all(np.isnan(res[i][1])) and np.all(np.isnan(res[i][2])) and np.all(np.isnan(res[i][3])), i
        assert res[i][1].shape == (len(seqs[i]), 4) and res[i][3].shape == (len(seqs[i]) + 1, 4), i
    for i in (0, 4, 6):
        assert _same_results(res[i], call["per_read"][True][i]), i
    for i, text in ((2, "empty"), (3, "too long for k_map_edits"), (5, "too short"), (7, "shorter than the model's k-mer")):
        eng.score_edits_transducer(sigs[i:i + 1], seqs[i:i + 1])
        assert text in sa.last_error(), (i, sa.last_error())
    ok = eng.score_edits_transducer(sigs[3:4], [seqs[3][:-1]][:1], viterbi=True)        # the longest sequence: scored (all A: most edits admit no path)
    assert ok[0][1].shape == (len(seqs[3]) - 1, 4) and not np.isnan(ok[0][0])


def test_crf_model_is_refused(eng, call):
    with pytest.raises(RuntimeError, match="rnnrf_r94.*flip-flop"):
        eng.score_edits_transducer(call["sigs"][:2], "ACGTACGTAC", model="rnnrf_r94")
    assert "scrappie_hip_map_crf_edits_batch" in sa.last_error()
    with pytest.raises(RuntimeError, match="rgrgr_r94.*transducer"):          # score_edits as it was
        eng.score_edits(call["sigs"][:2], "ACGTACGTAC", model=TR)


@pytest.mark.parametrize("viterbi", [True, False])
def test_the_highest_edits_scored_again_by_the_exact_engine(eng, call, worst, viterbi):
    """one read: the 20 highest edits by score_edits_transducer through map_post_to_sequences, within 2 |np32 - f64| + 1e-5 |f64|"""
    i = 4
    post, seq = call["posts"][i], call["calls"][i]
    (res,) = eng.score_edits_transducer([call["sigs"][i]], [seq], viterbi=viterbi)
    edits = all_edits(len(seq))
    sc = np.array([pick(res, *e) for e in edits], dtype=np.float64)
    order = [k for k in np.argsort(-np.where(np.isnan(sc), -np.inf, sc), kind="stable") if np.isfinite(sc[k])][:20]
    assert len(order) == 20
    edited = [sa.apply_edit(seq, *edits[k]) for k in order]
    again = sa.map_post_to_sequences(call["mats"][i], [_str(e) for e in edited], viterbi=viterbi)
    for k, ed, ag in zip(order, edited, again):
        f32 = float(np_map(post, encode(ed, 5), 0.0, 0.0, 4.0, viterbi=viterbi, dtype=np.float32)[0])
        f64 = float(np_map(post, encode(ed, 5), 0.0, 0.0, 4.0, viterbi=viterbi, dtype=np.float64)[0])
        bound = 2 * abs(f32 - f64) + 1e-5 * abs(f64)
        err = abs(sc[k] - float(ag))
        print("%s %r: edits %.9g exact %.9g f64 %.12g ratio %.3f" % ("viterbi" if viterbi else "forward", edits[k], sc[k], ag, f64, err / (bound + 1e-30)))
        assert err <= bound, (edits[k], sc[k], ag, f64)
        worst["cross"] = max(worst["cross"], err / (bound + 1e-30))


def test_seqmappy_kmer_edits_cli(eng, weights, tmp_path):
    """`scrappie seqmappy --kmer-edits` on a bundled read and a piece of its own call: what Engine.score_edits_transducer gives; the
    refusals name the option and print nothing"""
    f5 = os.path.join(READS, READ + ".i16")
    x = _prepared(f5)
    own = _codes(eng.basecall([x], TR)[0]["bases"])
    seq = np.concatenate([own, np.random.default_rng(5).integers(0, 4, 300)]).astype(np.int32)[:300]      # 300 bases that begin with the read's call (a single k-mer with synthetic weights)
    assert len(own) >= 5
    fa = str(tmp_path / "draft.fa")
    with open(fa, "w") as fh:
        fh.write(">draft\n%s\n" % _str(seq))
    crf_file, tr_file = str(tmp_path / "rnnrf_r94.scrm"), str(tmp_path / "rgrgr_r94.scrm")
    model.save_model(weights[0], crf_file)
    model.save_model(weights[1], tr_file)
    ((base, sub, dele, ins),) = eng.score_edits_transducer([x], [seq], viterbi=True)
    nblock = eng.read_blocks(TR, len(x))
    L = len(seq)

    def f(v):
        d = np.float32(v) - np.float32(base)
        return "nan" if np.isnan(d) else "%f" % d
    want = "# %s to %s -- edits of %d bases, score %f over %d blocks\n" % (f5, fa, L, base, nblock)
    want += "pos\tbase\tdel\tsubA\tsubC\tsubG\tsubT\tinsA\tinsC\tinsG\tinsT\n"
    for i in range(L):
        want += "\t".join(["%d" % i, "ACGT"[seq[i]], f(dele[i])] + [f(v) for v in sub[i]] + [f(v) for v in ins[i]]) + "\n"
    want += "\t".join(["%d" % L] + ["-"] * 6 + [f(v) for v in ins[L]]) + "\n"
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--kmer-edits", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    # three pairs: a fasta that is not there, the good pair, a sequence too long -- the good pair's lines, and each failure under its own name and reason
    long_fa = str(tmp_path / "long.fa")
    with open(long_fa, "w") as fh:
        fh.write(">long\n%s\n" % ("ACGT" * (sa.lib().scrappie_hip_map_edits_max_bases(5) // 4 + 1)))
    missing = str(tmp_path / "missing.fa")
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--kmer-edits", missing, f5, fa, f5, long_fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout == want, r.stderr
    lines = r.stderr.splitlines()
    assert any("missing.fa" in ln for ln in lines) and not any("draft.fa" in ln for ln in lines), r.stderr
    assert [("too long for --kmer-edits" in ln) for ln in lines if "long.fa" in ln] == [True], r.stderr
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--model-file", crf_file, "--kmer-edits", fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--kmer-edits" in r.stderr and "--edits" in r.stderr.replace("--kmer-edits", "") and r.stdout == ""
    r = subprocess.run([CLI, "seqmappy", "--model-file", tr_file, "--edits", fa, f5], capture_output=True, text=True, timeout=120)       # as it was
    assert r.returncode != 0 and "--edits" in r.stderr and r.stdout == ""


def test_every_map_edits_form_was_launched(forms_at_start, worst):
    """the last test of the module: each of the 8 k_map_edits_rows instantiations (Viterbi / forward x dense / tiled x forward /
    backward rows) and of the 4 k_map_edits ones has been launched by the tests above"""
    now = sa.map_edits_form_counts()
    ran = {k: now[k] - forms_at_start[k] for k in now}
    print("launches by form: %r" % sorted(ran.items()))
    print("forward: worst |gpu - f64| / (2 |np32 - f64| + 1e-5 |f64|) = %.3f per read, %.3f on the edits scored again" % (worst["per_read"], worst["cross"]))
    assert len(ran) == 12 and all(v > 0 for v in ran.values()), ran
