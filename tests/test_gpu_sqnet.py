"""Squiggle prediction on the GPU (sh_sqnet.h, k_sqnet): the per-read squiggle_r94 / squiggle_r94_rna, the batched
Engine.predict_squiggle, mappy as a composition with the squiggle matcher, and the two command lines, against the
references and the tolerance of tests/test_sqnet_cpu.py: every output column within 4 x E32 of the float64
restatement (E32: the float32 oracle's own distance from it).

The network tests run on the variants of tests/test_sqnet_cpu.py: the plain synthetic weights, the saturated ones (tanh
arguments to beyond 20, as the shipped models have them) and, for the activation alone, the sweep weights under which the
output is tanh of a known argument.  A variant goes on the engines under its model's name for the length of one test
(`variant_loaded`); the plain weights are back afterwards."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
import test_sqnet_cpu
from scrappie_amd import model
from test_sqnet_cpu import CLI, GPU_TOL_OF, MODELS, ROOT, VARIANTS, halo, references, tile, variant_weights, weights

pytestmark = pytest.mark.gpu

LETTERS = np.array(list("ACGT"))
READ = "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand"


def letters(codes):
    return "".join(LETTERS[np.asarray(codes)])


@pytest.fixture(scope="module")
def model_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sqnet_models")
    out = {}
    for name in MODELS:
        out[name] = str(d / (name + ".scrm"))
        model.save_model(weights(name), out[name])
    return out


@pytest.fixture(scope="module")
def registered(model_files):
    """both models on the process-default engine, under the names the per-read functions look for"""
    for name, path in model_files.items():
        sa.register_model(name, path)
    return model_files


@pytest.fixture(scope="module")
def eng(model_files):
    e = sa.Engine(0)
    for name, path in model_files.items():
        e.load_model(name, path)
    yield e
    e.close()


@pytest.fixture(scope="module")
def variant_files(tmp_path_factory, model_files):
    """{(model name, variant): file}"""
    d = tmp_path_factory.mktemp("sqnet_variants")
    out = {}
    for name in MODELS:
        for variant in VARIANTS:
            if variant == "plain":
                out[name, variant] = model_files[name]
            else:
                out[name, variant] = str(d / ("%s.%s.scrm" % (name, variant)))
                model.save_model(variant_weights(name, variant), out[name, variant])
    return out


@contextlib.contextmanager
def variant_loaded(name, variant, files, eng=None):
    """the variant's weights under the model's name, on the process-default engine and on `eng`; the plain ones afterwards"""
    try:
        if variant != "plain":
            sa.register_model(name, files[name, variant])
            if eng is not None:
                eng.load_model(name, files[name, variant])
        yield
    finally:
        if variant != "plain":
            sa.register_model(name, files[name, "plain"])
            if eng is not None:
                eng.load_model(name, files[name, "plain"])


def cases_of(variants):
    """(model, variant) for parametrize; the plain cases keep the ids they have always had"""
    return [pytest.param(name, v, id=name if v == "plain" else "%s-%s" % (name, v)) for v in variants for name in sorted(MODELS)]


_per_read = {}


def per_read(name, registered, variant="plain"):
    """{case name: (n, 3) float32} through the per-read function (a batch of one each), computed once; the variant's weights
    must be the registered ones (variant_loaded)"""
    if (name, variant) not in _per_read:
        got = {}
        for cn, (codes, r32, r64) in references(name, variant).items():
            m = sa.sequence_to_squiggle(letters(codes), model=name, rescale=False)
            mat = m.data().contents
            assert (mat.nr, mat.nrq, mat.nc, mat.stride) == (3, 1, len(codes), 4), cn
            padded = np.ctypeslib.as_array(C.cast(mat.data, C.POINTER(C.c_float)), shape=(mat.nc, 4))
            assert np.all(padded[:, 3] == 0.0), cn                         # pad lane
            got[cn] = m.data(as_numpy=True, sloika=False)
        _per_read[name, variant] = got
    return _per_read[name, variant]


@pytest.mark.parametrize("name,variant", cases_of(VARIANTS))
def test_per_read_against_float64(name, variant, registered, variant_files):
    tol = GPU_TOL_OF[variant]
    with variant_loaded(name, variant, variant_files):
        got_all = per_read(name, registered, variant)
    errs = {}
    for cn, (codes, r32, r64) in references(name, variant).items():
        got = got_all[cn]
        assert got.shape == (len(codes), 3) and got.dtype == np.float32, cn
        errs[cn] = np.max(np.abs(got.astype(np.float64) - r64), axis=0)
        print("%s %s %s: max |gpu - f64| per column %r" % (name, variant, cn, tuple(float(x) for x in errs[cn])))
    worst = np.max(list(errs.values()), axis=0)
    print("%s %s: worst per column %r of %r allowed" % (name, variant, tuple(float(x) for x in worst), tol))
    for cn, (codes, r32, r64) in references(name, variant).items():
        for k in range(3):
            assert errs[cn][k] <= tol[k], (cn, k, errs[cn][k], tol[k])
        if variant == "sweep":
            # the output is a tanh: never beyond +-1, and exactly +-1 wherever the float32 oracle's is
            got = got_all[cn]
            assert np.all(np.abs(got) <= 1.0), cn
            flat = np.abs(r32[:, 2]) == 1.0
            assert np.count_nonzero(flat) > len(codes) // 2 and np.array_equal(got[flat, 2], r32[flat, 2]), cn


@pytest.mark.parametrize("name,variant", cases_of(("plain", "saturated")))
def test_batch_is_bit_identical_to_per_read(name, variant, registered, eng, variant_files):
    with variant_loaded(name, variant, variant_files, eng):
        _batch_is_bit_identical_to_per_read(name, variant, registered, eng)


def _batch_is_bit_identical_to_per_read(name, variant, registered, eng):
    wl = MODELS[name][0]
    refs = references(name, variant)
    names = sorted(refs)
    np.random.RandomState(5).shuffle(names)
    seqs = [refs[cn][0] for cn in names]
    short = np.zeros(wl - 2, dtype=np.int32)
    bad = refs["random_49"][0].copy()
    bad[20] = 4
    mid = len(seqs) // 2
    seqs = seqs[:mid] + [short, bad] + seqs[mid:]
    names = names[:mid] + [None, None] + names[mid:]
    before = sa.lib().scrappie_hip_sqnet_launch_count()
    got = eng.predict_squiggle(seqs, model=name)
    assert sa.lib().scrappie_hip_sqnet_launch_count() == before + 1       # one launch over all tiles
    assert "shorter" in sa.last_error()                                   # the first refusal is the one reported
    for cn, g in zip(names, got):
        if cn is None:
            assert g is None
        else:
            assert g is not None and g.tobytes() == per_read(name, registered, variant)[cn].tobytes(), cn
    # launches cut by device memory: the same bits from several launches
    eng.debug_option("sqnet_budget_kb", 16)
    try:
        cut = eng.predict_squiggle(seqs, model=name)
        assert sa.lib().scrappie_hip_sqnet_launch_count() > before + 2
        for cn, g, c in zip(names, got, cut):
            assert (g is None and c is None) or g.tobytes() == c.tobytes(), cn
        t = eng.sqnet_timing()
        assert t["net_ms"] > 0 and t["upload_ms"] > 0 and t["download_ms"] > 0
    finally:
        eng.debug_option("sqnet_budget_kb", 0)


def test_failed_launch(eng):
    """the second of three launches refused (debug option fail_run): the call fails with that text and hands nothing back,
    and the engine then gives what it gave before.  A sequence of 300 bases takes 3996 bytes of a launch: four to a
    launch of 16 KB, twelve sequences in three launches."""
    name = sorted(MODELS)[0]
    rng = np.random.RandomState(9)
    seqs = [rng.randint(0, 4, 300).astype(np.int32) for _ in range(12)]
    count = sa.lib().scrappie_hip_sqnet_launch_count
    eng.debug_option("sqnet_budget_kb", 16)
    try:
        before = count()
        first = eng.predict_squiggle(seqs, model=name)
        assert count() == before + 3
        assert all(g is not None and g.shape == (300, 3) for g in first)
        eng.debug_option("fail_run", 2)
        got = None
        with pytest.raises(RuntimeError, match="injected failure"):
            got = eng.predict_squiggle(seqs, model=name)
        assert got is None
        assert count() == before + 4                       # the first launch ran, the second was refused, no third
        eng.debug_option("fail_run", 0)
        again = eng.predict_squiggle(seqs, model=name)
        assert all(a is not None and a.tobytes() == g.tobytes() for a, g in zip(again, first))
    finally:
        eng.debug_option("fail_run", 0)
        eng.debug_option("sqnet_budget_kb", 0)


@pytest.mark.parametrize("name,variant", cases_of(("plain", "saturated")))
def test_tile_seams(name, variant, registered, eng, variant_files):
    """around each tile edge of a 2 TP + 1 sequence, every position equals bit for bit the same position of a run on a
    sub-sequence that holds its whole receptive field (and puts it at another offset of another tile).  With the saturated
    weights too: the halo columns are where a stale value would come in with the largest weight."""
    with variant_loaded(name, variant, variant_files, eng):
        _tile_seams(name, variant, registered, eng, halo(MODELS[name][0]))


def _tile_seams(name, variant, registered, eng, h, slack=5):
    """h: the columns of context that a compared position needs to either side; the sub-sequences keep `slack` more"""
    tp = tile()
    codes = references(name, variant)["random_%d" % (2 * tp + 1)][0]
    full = per_read(name, registered, variant)["random_%d" % (2 * tp + 1)]
    subs, spans = [], []
    for seam in (tp, 2 * tp):
        lo, hi = seam - 3, min(seam + 3, len(codes))
        a, b = lo - h - slack, min(hi + h + slack, len(codes))
        subs.append(codes[a:b])
        spans.append((a, lo, hi if b - hi >= h or b == len(codes) else b - h))
    got = eng.predict_squiggle(subs, model=name)
    for (a, lo, hi), g in zip(spans, got):
        assert hi - lo >= 3
        assert g[lo - a:hi - a].tobytes() == full[lo:hi].tobytes(), (a, lo, hi)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_zero_layers_hand_their_input_through(name, registered, eng, variant_files):
    """The sweep weights: conv2..5 are all zeros, so each adds tanh(0) to its input, and conv6 is the identity on three
    filters.  The float32 oracle hands conv1's tanh through these five layers bit for bit (tests/test_sqnet_cpu.py,
    test_sweep_zero_layers_hand_their_input_through_on_the_oracle, and again below).  The kernel's conv1 stage cannot be read,
    so the same is asked of it through what follows from it: the output is then a function of one window of conv1 alone --
    the same bits per read, batched and from cut launches at 2 TP + 1 and 5 TP + 3, and around the tile seams the same bits
    from a sub-sequence that keeps only (WL - 1) / 2 columns of context, a sixth of what six live layers reach."""
    wl, tp = MODELS[name][0], tile()
    refs = references(name, "sweep")
    m = variant_weights(name, "sweep")
    for cn, (codes, r32, r64) in refs.items():
        stages = []
        test_sqnet_cpu.ref32(m, codes, stages)
        assert r32.tobytes() == np.ascontiguousarray(stages[0][:, :3]).tobytes(), cn
    names = sorted(refs)
    assert set(names) == {"random_%d" % (2 * tp + 1), "random_%d" % (5 * tp + 3)}
    with variant_loaded(name, "sweep", variant_files, eng):
        want = per_read(name, registered, "sweep")
        got = eng.predict_squiggle([refs[cn][0] for cn in names], model=name)
        for cn, g in zip(names, got):
            assert g.tobytes() == want[cn].tobytes(), cn
        eng.debug_option("sqnet_budget_kb", 16)
        try:
            before = sa.lib().scrappie_hip_sqnet_launch_count()
            cut = eng.predict_squiggle([refs[cn][0] for cn in names], model=name)
            assert sa.lib().scrappie_hip_sqnet_launch_count() > before + 1
            for cn, g in zip(names, cut):
                assert g.tobytes() == want[cn].tobytes(), cn
        finally:
            eng.debug_option("sqnet_budget_kb", 0)
        _tile_seams(name, "sweep", registered, eng, (wl - 1) // 2, slack=0)


def test_rescale_is_libm_on_the_host(registered, eng):
    libm = C.CDLL("libm.so.6")
    libm.expf.restype = C.c_float
    libm.expf.argtypes = [C.c_float]
    name = "squiggle_r94"
    codes = references(name)["random_%d" % (tile() + 1)][0]
    plain = per_read(name, registered)["random_%d" % (tile() + 1)]
    scaled = sa.sequence_to_squiggle(letters(codes), model=name, rescale=True).data(as_numpy=True, sloika=False)
    want = plain.copy()
    want[:, 1] = [libm.expf(float(x)) for x in plain[:, 1]]
    want[:, 2] = [libm.expf(-float(x)) for x in plain[:, 2]]
    assert scaled.tobytes() == want.tobytes()
    assert eng.predict_squiggle([codes], model=name, rescale=True)[0].tobytes() == want.tobytes()


def _mappy_weights():
    """the synthetic squiggle_r94 with an output layer that predicts a matchable squiggle: means of order 1, sd near 0.15, dwell near 8"""
    w = dict(weights("squiggle_r94"))
    w6 = w["conv6_W"].copy()
    w6[0] *= 4.0
    w6[1:] *= 0.1
    w["conv6_W"] = w6
    w["conv6_b"] = np.array([0.0, np.log(0.15), np.log((1 / 8.0) / (1 - 1 / 8.0))], dtype=np.float32)
    return w


def _sample_signal(params, seed):
    """as synth.simulated_squiggle samples from its parameters: Geometric(logistic(dwell logit)) samples per position, Laplace noise of the position's scale"""
    rng = np.random.RandomState(seed)
    p = 1.0 / (1.0 + np.exp(-params[:, 2].astype(np.float64)))
    truth = np.repeat(np.arange(len(params)), rng.geometric(p))
    sig = params[truth, 0] + rng.laplace(0.0, 1.0, size=len(truth)) * np.exp(params[truth, 1])
    return sig.astype(np.float32)


def test_mappy_is_predict_then_match(registered, eng, tmp_path):
    name = "squiggle_r94"
    mf = str(tmp_path / "mappy.scrm")
    model.save_model(_mappy_weights(), mf)
    lds = int(sa.lib().scrappie_hip_squiggle_lds_max_pos())
    rng = np.random.RandomState(77)
    seqs = [letters(rng.randint(0, 4, size=n)) for n in (lds - 40, lds + 3)]
    forms0 = sa.launch_form_counts()["squig"]
    try:
        eng.load_model(name, mf)
        sa.register_model(name, mf)
        sqs = eng.predict_squiggle(seqs, model=name)
        sigs = [_sample_signal(sq, 90 + i) for i, sq in enumerate(sqs)]
        want = eng.match_squiggle(sigs, sqs, viterbi=True, path=True)
        got = eng.mappy(sigs, seqs, model=name)
        for (ws, wp), (gs, gp), sig in zip(want, got, sigs):
            assert np.float32(ws).tobytes() == np.float32(gs).tobytes() and np.array_equal(wp, gp)
            assert np.isfinite(gs) and np.count_nonzero(gp >= 0) >= len(sig) / 2
        forms1 = sa.launch_form_counts()["squig"]
        assert forms1[(True, False)] > forms0[(True, False)] and forms1[(True, True)] > forms0[(True, True)]       # below and above the LDS threshold
        # the scrappy form: trim -> scale -> match against the per-read prediction
        raw = np.concatenate([sigs[0][:300], sigs[0]])
        gs, gp = sa.map_signal_to_squiggle(raw, seqs[0], model=name)
        rt = sa.RawTable(raw)
        rt.trim().scale()
        ws, wp = sa.squiggle_match(rt, sqs[0])
        assert np.float32(ws).tobytes() == np.float32(gs).tobytes() and np.array_equal(wp, gp) and len(gp) == len(raw)
    finally:
        eng.load_model(name, registered[name])
        sa.register_model(name, registered[name])


def _format_squiggle(name, seq, sq):
    lines = ["#%s" % name, "pos\tbase\tcurrent\tsd\tdwell"]
    lines += ["%d\t%s\t%3.6f\t%3.6f\t%3.6f" % (i, seq[i], sq[i, 0], sq[i, 1], sq[i, 2]) for i in range(len(seq))]
    return lines


def test_cli_squiggle(registered, eng, tmp_path):
    name = "squiggle_r94_rna"
    refs = references(name)
    recs = [("first", letters(refs["random_49"][0])), ("short", "ACGT"), ("third", letters(refs["random_%d" % (tile() + 1)][0]))]
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s some description\n%s\n%s\n" % (n, s[:30], s[30:]) for n, s in recs))
    for flag, rescale in ((None, True), ("--no-rescale", False)):
        cmd = [CLI, "squiggle", "-m", name, "--model-file", registered[name]] + ([flag] if flag else []) + [str(fa)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        sqs = eng.predict_squiggle([recs[0][1], recs[2][1]], model=name, rescale=rescale)
        want = _format_squiggle(recs[0][0], recs[0][1], sqs[0]) + _format_squiggle(recs[2][0], recs[2][1], sqs[1])
        assert r.stdout.splitlines() == want
    r = subprocess.run([CLI, "squiggle", "-m", name, "--model-file", registered[name], "-l", "1", str(fa)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines() == _format_squiggle(recs[0][0], recs[0][1], eng.predict_squiggle([recs[0][1]], model=name, rescale=True)[0])


def test_cli_mappy(registered, eng, fast5_dir):
    name = "squiggle_r94"
    fa = os.path.join(ROOT, "tests", "golden", "reads", READ + ".fa")
    f5 = os.path.join(fast5_dir, READ + ".fast5")
    seq = "".join(l.strip() for l in open(fa).read().splitlines()[1:])
    L = sa.lib()
    L.scrappie_hip_read_raw.restype = sa._RawTable
    L.scrappie_hip_read_raw.argtypes = [C.c_char_p, C.c_bool]
    rt = L.scrappie_hip_read_raw(os.fsencode(f5), True)
    raw = np.ctypeslib.as_array(rt.raw, shape=(rt.n,)).copy()
    sa._libc.free(C.cast(rt.raw, C.c_void_p))
    score, path = sa.map_signal_to_squiggle(raw, seq, model=name)
    r = subprocess.run([CLI, "mappy", "--model-file", registered[name], fa, f5], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "# %s to %s  (score = %f)" % (f5, fa, score)
    assert lines[1] == "idx\tsignal\tpos\tbase\tcurrent\tsd\tdwell" and len(lines) == 2 + len(raw)
    pos = np.array([int(l.split("\t")[2]) for l in lines[2:]])
    assert np.array_equal(pos, path)
    bases = [l.split("\t")[3] for l in lines[2:]]
    assert all(b == ("N" if p < 0 else seq[p]) for b, p in zip(bases, pos))
