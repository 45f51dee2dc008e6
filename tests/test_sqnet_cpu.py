"""The squiggle-predicting network (sh_sqnet.h; networks.c:397-565), everything that needs no GPU: two references for the
GPU tests (tests/test_gpu_sqnet.py imports them), the tolerance they hold the kernel to, the model container, the
argument checks of the per-read functions and the plumbing of `scrappie squiggle` / `scrappie mappy`.

ref32  the network composed from what liboracle.so exports: a numpy gather for the embedding, orc_convolution (pinned on
       the reference's own convolution vectors by tests/test_oracle_golden.py) with the weights in the reference's padded
       layout, orc_tanh_activation_inplace, a numpy float32 add for the residual.
ref64  an independent float64 restatement from networks.c / layers.c: zero-padded "same" convolution, np.tanh.

Tolerance of the GPU tests: per output column, 4 x E32 against ref64, where E32 = max |ref32 - ref64| over all the cases
below -- the float32 oracle against float64, never the code under test.  The oracle's summation order is one order of
many; the project has measured up to 2x between two orders of the same sums, and the factor is twice that.

Three variants of each model's weights, each with its own references and its own E32:
plain      model.synthetic_model as it is.  Its pre-activations stay below about 4.5: the near-linear part and the knee of tanh.
saturated  conv1..conv5 W times GAINS[name].  A quarter to a half of conv4 / conv5 pre-activations lie beyond |x| = 4 and the largest
           beyond 20, as in the shipped models (test_saturated_variant_is_in_the_shipped_regime, ..._brackets_the_shipped_models).
sweep      designed weights: the output IS tanh(pre-activation of conv1) in three columns whose arguments sweep [-1.5, 1.5],
           [-7.5, 7.5] and [-30, 30] evenly (sweep_weights), so the kernel's tanh is compared value by value.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import scrappie_amd as sa
from scrappie_amd import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
PM = C.POINTER(sa._Mat)

# name -> (window, seed of the synthetic weights)
MODELS = {"squiggle_r94": (9, 11), "squiggle_r94_rna": (7, 12)}

# max |ref32 - ref64| per output column (mean, log sd, dwell logit) over sqnet_cases() of both models, measured by
# test_e32_is_what_the_oracle_gives (which holds these to the measurement); also in DESIGN.md
E32 = (3.45e-6, 3.30e-6, 2.65e-6)
GPU_TOL = tuple(4.0 * e for e in E32)

VARIANTS = ("plain", "saturated", "sweep")
# what saturated_weights multiplies conv1_W .. conv5_W by.  The RNA model's conv3 takes 2.5 where the other takes 2: the shipped
# squiggle_r94_rna reaches 7.9 in conv3, which a gain of 2 (6.8) does not bracket (test_saturated_variant_brackets_the_shipped_models)
GAINS = {"squiggle_r94": (1.0, 1.5, 2.0, 3.0, 4.0), "squiggle_r94_rna": (1.0, 1.5, 2.5, 3.0, 4.0)}
# the same measurement over the cases of the saturated and of the sweep variant (variant_cases), held by the same test
E32_SAT = (4.85e-6, 6.86e-6, 3.84e-6)
E32_SWEEP = (1.67e-7, 1.71e-7, 2.76e-7)
E32_OF = {"plain": E32, "saturated": E32_SAT, "sweep": E32_SWEEP}
GPU_TOL_OF = {v: tuple(4.0 * e for e in E32_OF[v]) for v in VARIANTS}


def tile():
    """output positions per workgroup of k_sqnet: host only, works without a device"""
    return int(sa.lib().scrappie_hip_sqnet_tile())


def halo(wl):
    """how far one base reaches through six windows"""
    return 6 * ((wl - 1) // 2)


_weights = {}


def weights(name):
    if name not in _weights:
        _weights[name] = model.synthetic_model(name, seed=MODELS[name][1])
    return _weights[name]


def saturated_weights(name):
    """weights(name) with conv1_W .. conv5_W times GAINS[name] (float32); biases, embedding and conv6 as they are"""
    m = dict(weights(name))
    for l, g in enumerate(GAINS[name], 1):
        m["conv%d_W" % l] = (m["conv%d_W" % l] * np.float32(g)).astype(np.float32)
    return m


SWEEP_SCALES = (1.0, 5.0, 20.0)


def sweep_weights(name):
    """Weights under which output column k is tanh(SWEEP_SCALES[k] * s), s spread evenly over [-1.5, 1.5).

    embedding  feature 0 of base d = 0..3 is (2 d - 3) / 3: four equally spaced digits, -1 .. 1 (features 1, 2 as in weights(name)).
    conv1      filters 0, 1, 2 live, every other filter and every bias zero.  Filter 0 reads feature 0 only, tap number r in the
               order centre, +1, -1, +2, -2 ... with weight 1.5 * 3/4 * 4^-r: the window's bases are the digits of a number in
               base 4, so s = 1.5 (2 u - 1) with u uniform on [0, 1) over random bases.  Filters 1 and 2 are 5 and 20 times that.
    conv2..5   W = 0, b = 0: each adds tanh(0) = 0 to its input and hands it on.
    conv6      the centre tap, identity on filters 0..2, b = 0."""
    wl = MODELS[name][0]
    pad = (wl - 1) // 2
    m = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in weights(name).items()}
    m["embed_W"][:, 0] = (2.0 * np.arange(4) - 3.0) / 3.0
    order = [pad] + [pad + sgn * k for k in range(1, pad + 1) for sgn in (1, -1)]
    base = np.zeros((wl, 3))
    base[order, 0] = 1.5 * 0.75 * 4.0 ** -np.arange(wl)
    for l in range(1, 7):
        m["conv%d_W" % l] = np.zeros_like(m["conv%d_W" % l])
        m["conv%d_b" % l] = np.zeros_like(m["conv%d_b" % l])
    for k, sc in enumerate(SWEEP_SCALES):
        m["conv1_W"][k] = (sc * base).reshape(-1).astype(np.float32)
        m["conv6_W"][k, pad * 32 + k] = 1.0
    return m


_variant_weights = {}


def variant_weights(name, variant):
    if (name, variant) not in _variant_weights:
        _variant_weights[name, variant] = {"plain": weights, "saturated": saturated_weights, "sweep": sweep_weights}[variant](name)
    return _variant_weights[name, variant]


def sqnet_cases(name):
    """[(case name, int32 codes)]: the sizes of a single tile from the smallest defined one, the tile boundaries, a long
    one, and at 2 TP + 1 the four composition classes."""
    wl = MODELS[name][0]
    tp = tile()
    out = []
    sizes = [wl - 1, wl, wl + 1, 2 * wl, 47, 48, 49, tp - 1, tp, tp + 1, 2 * tp + 1, 5 * tp + 3]
    for k, n in enumerate(sizes):
        rng = np.random.RandomState(1000 * wl + k)
        out.append(("random_%d" % n, rng.randint(0, 4, size=n).astype(np.int32)))
    n = 2 * tp + 1
    base = dict(out)["random_%d" % n]
    out.append(("homopolymer_%d" % n, np.full(n, 2, dtype=np.int32)))
    out.append(("period2_%d" % n, np.tile(np.array([1, 3], dtype=np.int32), n // 2 + 1)[:n].copy()))
    one = base.copy()
    one[tp + 7] = (one[tp + 7] + 1) % 4
    out.append(("onebase_%d" % n, one))
    return out


def variant_cases(name, variant):
    """the cases of a variant: all of sqnet_cases, for the sweep the two long random ones (several tiles, 1404 positions)"""
    cases = sqnet_cases(name)
    if variant == "sweep":
        tp = tile()
        cases = [c for c in cases if c[0] in ("random_%d" % (2 * tp + 1), "random_%d" % (5 * tp + 3))]
        assert len(cases) == 2
    return cases


def _padded_filter(w, cin):
    """(cout, WL cin) -> the reference's layout: every tap's cin features padded to a multiple of 4, the last pad lanes dropped from nr"""
    cout, k = w.shape
    wl = k // cin
    cq = 4 * ((cin + 3) // 4)
    full = np.zeros((cout, wl, cq), dtype=np.float32)
    full[:, :, :cin] = w.reshape(cout, wl, cin)
    m = oracle.NpMat(full.reshape(cout, wl * cq)[:, :wl * cq - (cq - cin)])
    assert m.mat.stride == wl * cq
    return m


def ref32(m, codes, stages=None):
    """(n, 3) float32: the oracle's float32 composition; a list given as `stages` receives every layer's output"""
    L = oracle.lib()
    x = np.ascontiguousarray(m["embed_W"][np.asarray(codes)], dtype=np.float32)
    for l in range(1, 7):
        cin = x.shape[1]
        X, W, b = oracle.NpMat(x), _padded_filter(m["conv%d_W" % l], cin), oracle.NpMat(m["conv%d_b" % l].reshape(1, -1))
        c = L.orc_convolution(X.ptr, W.ptr, b.ptr, 1, None)
        assert c
        if l < 6:
            L.orc_tanh_activation_inplace(c)
        y = oracle.mat_to_numpy(c, free_with=L.orc_free_mat)
        x = (y + x).astype(np.float32) if 2 <= l <= 5 else y
        if stages is not None:
            stages.append(x)
    return x


def _conv64(x, w, b):
    n, cin = x.shape
    wl = w.shape[1] // cin
    pad = (wl - 1) // 2
    xp = np.zeros((n + wl - 1, cin), dtype=np.float64)
    xp[pad:pad + n] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, wl, axis=0)          # (n, cin, wl)
    win = win.transpose(0, 2, 1).reshape(n, wl * cin)                       # column = tap * cin + feature
    return win @ w.astype(np.float64).T + b.astype(np.float64)


def ref64(m, codes, pre=None):
    """(n, 3) float64: embedding, tanh(conv1), four times tanh(conv(x)) + x, conv6; a list given as `pre` receives the
    argument of tanh of conv1 .. conv5, (n, 32) each"""
    x = m["embed_W"].astype(np.float64)[np.asarray(codes)]
    for l in range(1, 6):
        p = _conv64(x, m["conv%d_W" % l], m["conv%d_b" % l])
        if pre is not None:
            pre.append(p)
        x = np.tanh(p) + x if l > 1 else np.tanh(p)
    return _conv64(x, m["conv6_W"], m["conv6_b"])


_refs = {}


def references(name, variant="plain"):
    """{case name: (codes, ref32, ref64)} of a model variant, computed once per process"""
    if (name, variant) not in _refs:
        m = variant_weights(name, variant)
        _refs[name, variant] = {cn: (codes, ref32(m, codes), ref64(m, codes)) for cn, codes in variant_cases(name, variant)}
    return _refs[name, variant]


def test_e32_is_what_the_oracle_gives():
    for variant in VARIANTS:
        worst = np.zeros(3)
        for name in MODELS:
            for cn, (codes, r32, r64) in references(name, variant).items():
                assert r32.shape == r64.shape == (len(codes), 3) and r32.dtype == np.float32
                assert np.all(np.isfinite(r64)) and float(np.std(r64[:, 0])) > 0.05, cn       # the cases say something
                worst = np.maximum(worst, np.max(np.abs(r32.astype(np.float64) - r64), axis=0))
        print("E32 measured, %s: %r" % (variant, tuple(float(x) for x in worst)))
        for k in range(3):
            assert 0.9 * E32_OF[variant][k] <= worst[k] <= E32_OF[variant][k], (variant, k, worst[k], E32_OF[variant][k])


def regime(m, seqs):
    """over the sequences, on ref64: (max |argument of tanh| per layer conv1..conv5, share of arguments beyond |x| = 4 per layer, max |output|)"""
    top, beyond, count, out = np.zeros(5), np.zeros(5), 0, 0.0
    for codes in seqs:
        pre = []
        out = max(out, float(np.max(np.abs(ref64(m, codes, pre)))))
        for l, p in enumerate(pre):
            top[l] = max(top[l], float(np.max(np.abs(p))))
            beyond[l] += np.count_nonzero(np.abs(p) > 4.0)
        count += pre[0].size
    return top, beyond / count, out


def test_saturated_variant_is_in_the_shipped_regime():
    """On the cases themselves.  The plain weights leave the part of tanh beyond |x| = 4 practically unvisited (conv5: under one
    argument in a thousand, none beyond 4.6); the saturated ones put a quarter to a half of conv4 / conv5 there and reach
    beyond 20, which is where the shipped models run (DESIGN.md 5d has the table)."""
    for name in sorted(MODELS):
        seqs = [codes for cn, codes in sqnet_cases(name)]
        top, share, out = regime(variant_weights(name, "plain"), seqs)
        print("%s plain:     max |pre| %s  share beyond 4 %s  max |out| %.2f" % (name, np.round(top, 2), np.round(share, 5), out))
        assert share[4] < 0.001, (name, share)
        top, share, out = regime(variant_weights(name, "saturated"), seqs)
        print("%s saturated: max |pre| %s  share beyond 4 %s  max |out| %.2f" % (name, np.round(top, 2), np.round(share, 5), out))
        assert 0.25 <= share[4] <= 0.7, (name, share)
        assert share[3] >= 0.1, (name, share)
        assert np.max(top) >= 20.0, (name, top)
        assert variant_weights(name, "saturated")["conv3_W"].dtype == np.float32
        for nm in ("embed_W", "conv6_W", "conv6_b") + tuple("conv%d_b" % l for l in range(1, 6)):
            assert np.array_equal(variant_weights(name, "saturated")[nm], weights(name)[nm]), nm


SHIPPED = (("squiggle_r94.h", "squiggle_r94"), ("squiggle_r94_rna.h", "squiggle_r94_rna"), ("squiggle_r10.h", "squiggle_r94"))


@pytest.mark.parametrize("header,name", SHIPPED, ids=[h[:-2] for h, _ in SHIPPED])
def test_saturated_variant_brackets_the_shipped_models(header, name):
    """On 2000 random bases: in every layer the saturated variant of the same window reaches at least as far as the shipped
    model, and at least as large a share of its conv5 arguments lies beyond |x| = 4.

    This is what sets GAINS.  With (1, 1.5, 2, 3, 4) for both models squiggle_r94 and squiggle_r10 are bracketed, but the RNA
    variant reaches 6.76 in conv3 where the shipped squiggle_r94_rna reaches 7.92; with 2.5 in conv3 it reaches 8.47."""
    d = "/root/reference/src/models"
    if not os.path.isdir(d):
        pytest.skip("no reference checkout")
    seqs = [np.random.RandomState(0).randint(0, 4, size=2000).astype(np.int32)]
    top_s, share_s, _ = regime(model.squiggle_model_from_header(os.path.join(d, header)), seqs)
    top, share, _ = regime(variant_weights(name, "saturated"), seqs)
    print("%s: max |pre| %s  conv5 share beyond 4 %.4f" % (header, np.round(top_s, 2), share_s[4]))
    print("%s saturated: max |pre| %s  conv5 share beyond 4 %.4f" % (name, np.round(top, 2), share[4]))
    for l in range(5):
        assert top[l] >= top_s[l], (header, "conv%d" % (l + 1), top[l], top_s[l])
    assert share[4] >= share_s[4], (header, share[4], share_s[4])


@pytest.mark.parametrize("name", sorted(MODELS))
def test_sweep_covers_the_range_of_tanh(name):
    """the arguments of the three live tanh of the sweep variant, on ref64, over its cases: at least 3 positions in every
    unit-wide bin of [-25, 25] (column 2) and in every 0.1-wide bin of [-1, 1] (column 0); nothing else is live"""
    m = variant_weights(name, "sweep")
    pre1 = []
    for cn, (codes, r32, r64) in references(name, "sweep").items():
        pre = []
        out = ref64(m, codes, pre)
        assert np.array_equal(out, np.tanh(pre[0][:, :3])), cn
        assert not np.any(pre[0][:, 3:]) and all(not np.any(p) for p in pre[1:]), cn
        pre1.append(pre[0][:, :3])
    pre1 = np.concatenate(pre1)
    print("%s: arguments span %s .. %s" % (name, np.round(pre1.min(axis=0), 2), np.round(pre1.max(axis=0), 2)))
    for k, reach in enumerate((1.5, 7.5, 30.0)):
        assert 0.9 * reach < np.max(pre1[:, k]) < reach and -reach < np.min(pre1[:, k]) < -0.9 * reach
    wide = np.histogram(pre1[:, 2], bins=50, range=(-25.0, 25.0))[0]
    fine = np.histogram(pre1[:, 0], bins=20, range=(-1.0, 1.0))[0]
    assert wide.min() >= 3 and fine.min() >= 3, (wide, fine)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_sweep_zero_layers_hand_their_input_through_on_the_oracle(name):
    """ref32 of the sweep weights is, bit for bit, what the oracle's conv1 + tanh stage gives in filters 0..2: its tanh(0)
    is 0 and the residual adds and the identity tap of conv6 are exact.  (tests/test_gpu_sqnet.py asks the same of the kernel.)"""
    m = variant_weights(name, "sweep")
    for cn, (codes, r32, r64) in references(name, "sweep").items():
        stages = []
        assert ref32(m, codes, stages).tobytes() == r32.tobytes()
        assert r32.tobytes() == np.ascontiguousarray(stages[0][:, :3]).tobytes(), cn
        assert not np.any(stages[0][:, 3:]) and np.max(np.abs(r32)) <= 1.0


@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_base_reaches_six_windows_and_no_further(name):
    """the receptive field, on ref64: a changed base moves the output within 6 (WL - 1) / 2 positions of it, and all the way out to there"""
    wl = MODELS[name][0]
    tp = tile()
    refs = references(name)
    n = 2 * tp + 1
    a, b = refs["random_%d" % n][2], refs["onebase_%d" % n][2]
    moved = np.nonzero(np.any(a != b, axis=1))[0]
    assert moved.min() >= tp + 7 - halo(wl) and moved.max() <= tp + 7 + halo(wl)
    assert moved.min() <= tp + 7 - halo(wl) + 2 and moved.max() >= tp + 7 + halo(wl) - 2


def test_ref64_pads_every_layer_with_zeros():
    """the property the fused kernel must keep: the first positions see zeros, not tanh(bias), beyond the sequence's start --
    a sequence and the same sequence behind a long prefix differ there"""
    m = weights("squiggle_r94")
    codes = references("squiggle_r94")["random_49"][0]
    alone = ref64(m, codes)
    behind = ref64(m, np.concatenate([np.zeros(40, dtype=np.int32), codes]))[40:]
    assert np.max(np.abs(alone[:halo(9)] - behind[:halo(9)])) > 1e-3
    assert np.array_equal(alone[halo(9):], behind[halo(9):]) or np.max(np.abs(alone[halo(9):] - behind[halo(9):])) < 1e-12


def test_scrm_round_trip(tmp_path):
    for name in MODELS:
        m = weights(name)
        p = str(tmp_path / (name + ".scrm"))
        model.save_model(m, p)
        back = model.load_model(p)
        assert back["arch"] == "squiggle" and back["conv_act"] == "tanh" and back["stride"] == 1
        assert model.matrix_names(back) == model.SQUIGGLE_MATRIX_NAMES
        for nm in model.SQUIGGLE_MATRIX_NAMES:
            assert back[nm].dtype == np.float32 and back[nm].shape == m[nm].shape and np.array_equal(back[nm], m[nm]), nm
        assert model.model_dims(back)["WL"] == MODELS[name][0]
    assert model.MODEL_SHAPES["squiggle_r10"][2] == 9 and model.MODEL_SHAPES["squiggle_r94_rna"][2] == 7
    assert model.synthetic_model("squiggle_r10", seed=3)["conv6_W"].shape == (3, 32 * 9)


def test_squiggle_model_from_header_synthetic(tmp_path):
    """a header in the reference's format written from synthetic weights (3 features padded to 4 in conv1) reads back exactly"""
    m = weights("squiggle_r94_rna")
    wl = 7

    def emit(nm, a, nr):          # a: (nc, stride) padded rows
        vals = ", ".join(float(v).hex() for v in a.reshape(-1))
        return ("float __%s[%d] = {\n%s};\n_Mat _%s = {\n\t.nr = %d,\n\t.nrq = %d,\n\t.nc = %d,\n\t.stride = %d,\n\t.data.f = __%s\n};\n"
                % (nm, a.size, vals, nm, nr, a.shape[1] // 4, a.shape[0], a.shape[1], nm))

    text = emit("embed_t_W", np.pad(m["embed_W"], ((0, 0), (0, 1))), 3)
    c1 = np.pad(m["conv1_W"].reshape(32, wl, 3), ((0, 0), (0, 0), (0, 1))).reshape(32, 4 * wl)
    text += emit("conv1_t_W", c1, 4 * wl - 1) + emit("conv1_t_b", m["conv1_b"].reshape(1, -1), 32) + "const int conv1_t_stride = 1;\n"
    for l in range(2, 7):
        b = m["conv%d_b" % l]
        bp = np.pad(b, (0, (-len(b)) % 4)).reshape(1, -1)
        text += emit("conv%d_t_W" % l, m["conv%d_W" % l], 32 * wl) + emit("conv%d_t_b" % l, bp, len(b)) + "const int conv%d_t_stride = 1;\n" % l
    p = tmp_path / "squiggle_t.h"
    p.write_text(text)
    back = model.squiggle_model_from_header(str(p))
    for nm in model.SQUIGGLE_MATRIX_NAMES:
        assert np.array_equal(back[nm], m[nm]), nm


def test_squiggle_model_from_header_shipped():
    d = "/root/reference/src/models"
    if not os.path.isdir(d):
        pytest.skip("no reference checkout")
    for fn, wl in (("squiggle_r94.h", 9), ("squiggle_r94_rna.h", 7), ("squiggle_r10.h", 9)):
        m = model.squiggle_model_from_header(os.path.join(d, fn))
        assert m["embed_W"].shape == (4, 3) and m["conv1_W"].shape == (32, 3 * wl) and m["conv6_W"].shape == (3, 32 * wl), fn
        for l in range(2, 6):
            assert m["conv%d_W" % l].shape == (32, 32 * wl) and m["conv%d_b" % l].shape == (32,), (fn, l)
        assert model.model_dims(m)["WL"] == wl and m["conv6_b"].shape == (3,)
        assert np.all(np.isfinite(ref64(m, np.arange(40) % 4)))


def test_argument_errors_launch_nothing(monkeypatch):
    L = sa.lib()
    monkeypatch.delenv("SCRAPPIE_MODEL_DIR", raising=False)
    ip = C.POINTER(C.c_int)
    before = L.scrappie_hip_sqnet_launch_count()
    good = (np.arange(40) % 4).astype(np.int32)
    for fn, wl in ((L.squiggle_r94, 9), (L.squiggle_r94_rna, 7), (L.squiggle_r10, 9)):
        assert not fn(None, 100, False) and "no sequence" in sa.last_error()
        assert not fn(good.ctypes.data_as(ip), wl - 2, False) and "shorter" in sa.last_error()
        bad = good.copy()
        bad[17] = 4
        assert not fn(bad.ctypes.data_as(ip), len(bad), True) and "code 4 at base 17" in sa.last_error()
        bad[17] = -1
        assert not fn(bad.ctypes.data_as(ip), len(bad), True) and "outside 0..3" in sa.last_error()
    # squiggle_r10 is registered nowhere in the suite
    assert not L.squiggle_r10(good.ctypes.data_as(ip), len(good), False)
    assert "squiggle_r10" in sa.last_error() and "not registered" in sa.last_error()
    with pytest.raises(KeyError):
        sa.sequence_to_squiggle("ACGTACGTACGT", model="squiggle_r11")
    with pytest.raises(RuntimeError, match="not registered"):
        sa.sequence_to_squiggle("ACGTACGTACGT", model="squiggle_r10")
    with pytest.raises(RuntimeError):
        sa.sequence_to_squiggle("ACGTNCGTACGT", model="squiggle_r10")
    assert L.scrappie_hip_sqnet_launch_count() == before


def test_a_sequence_without_a_model_name_is_still_refused():
    with pytest.raises(NotImplementedError, match="model"):
        sa.map_signal_to_squiggle(np.zeros(1000, dtype=np.float32), "ACGTACGTACGT")


def test_pyscrap_squiggle_net_cdef_links(tmp_path):
    """include/pyscrap_squiggle_net.h: the three prototypes agree with scrappie_hip.h and link against the built library alone"""
    text = open(os.path.join(ROOT, "include", "pyscrap_squiggle_net.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    names = re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*\(", text)
    assert sorted(names) == ["squiggle_r10", "squiggle_r94", "squiggle_r94_rna"]
    src = tmp_path / "link.c"
    src.write_text('#include "scrappie_hip.h"\n' + text + "\nvoid *table[] = {" + ", ".join("(void *)" + n for n in names) +
                   "};\nint main(void) { return table[0] == 0; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "link"),
                        "-L", os.path.join(ROOT, "scrappie_amd"), "-lscrappie_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "scrappie_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "link")]).returncode == 0


def test_cli_plumbing(tmp_path):
    fa = tmp_path / "a.fa"
    fa.write_text(">one first\nACGTACGTACGTACGTACGT\nACGT\n>two\nACG\n")
    mf = str(tmp_path / "m.scrm")
    model.save_model(weights("squiggle_r94"), mf)
    f5 = os.path.join(ROOT, "tests", "golden", "reads", "read_ch228_file118.i16")
    r = subprocess.run([CLI, "events", "x"], capture_output=True, text=True)
    assert r.returncode != 0 and "not part of this build" in r.stderr
    for sub, opt in (("squiggle", "-m"), ("mappy", "--model")):
        r = subprocess.run([CLI, sub, opt, "squiggle_r95", "--model-file", mf, str(fa), f5], capture_output=True, text=True)
        assert r.returncode != 0 and "Invalid squiggle model name" in r.stderr, sub
        r = subprocess.run([CLI, sub], capture_output=True, text=True)
        assert r.returncode != 0 and "Usage: scrappie " + sub in r.stderr
    r = subprocess.run([CLI, "mappy", "--model-file", mf, str(fa)], capture_output=True, text=True)
    assert r.returncode != 0 and "fast5 file is a required argument" in r.stderr
    env = {k: v for k, v in os.environ.items() if k != "SCRAPPIE_MODEL_DIR"}
    r = subprocess.run([CLI, "squiggle", str(fa)], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "no weights for model squiggle_r94" in r.stderr
    if sa.lib().scrappie_hip_device_count() > 0:
        return
    for args in (["squiggle", "--model-file", mf, str(fa)], ["mappy", "--model-file", mf, str(fa), f5]):
        r = subprocess.run([CLI] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "HIP device" in r.stderr and r.stdout == "", args      # fails loudly, no CPU fallback
