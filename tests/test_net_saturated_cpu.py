"""The recurrent networks with their gates driven past saturation by the BIASES, against float64.

model.synthetic_model draws U(+-sqrt(3 / fan_in)) weights and U(+-0.1) biases: 98 % of the gate pre-activations of rgrgr_r94 lie below 2
and none beyond 8 (test_premise_...), so no test of the suite runs a gate outside the linear part of its activation, while shipped models
run theirs deep into saturation.  Scaling the recurrent weights up does not give a usable test (x 4 puts the layers into the chaotic regime,
where the fp32 oracle alone is 2 away from float64); a gate pinned by its bias has vanishing gain, the dynamics stay contractive and the
project's tolerances hold.  saturated_biases() adds one of LEVELS to every bias of the recurrent layers and of the feedforward2_tanh joins:
a fifth of the gates each stay linear (|pre| < 2), bend (2 - 8), saturate (8 - 17), give exactly 0 / 1 in fp32 (17 - 88.4: 1 + e == 1) and
pass the clamp of the exponential (>= 88.4, where the clamped and the clamp-free forms of the kernels part ways).

This module holds the variant, the float64 statement of every layer of every graph on it (composed from the functions of
tests/golden/make_net_f64.py, computed at test time, shared with tests/test_gpu_net_saturated.py), and the CPU tests:

  * the premise (plain synthetic weights never saturate) and the census of the variant (every band is populated in every graph);
  * oracle.c against the float64 statement on the variant, for every case the GPU tests use, within HALF of each tolerance of
    tests/test_net_f64.py -- the condition under which a GPU result outside the full tolerance is the kernels' error, not the statement's.
"""
import functools
import re

import numpy as np
import pytest

import make_net_f64 as F
from scrappie_amd import model, synth

from test_net_f64 import P_TOL, LOGP_TOL, ACT_TOL, CRF_TOL

LEVELS = [0, 0, 4, -4, 10, -10, 30, -30, 120, -120]
BANDS = (0.0, 2.0, 8.0, 17.0, 88.4, np.inf)         # linear | bending | saturated | exactly 0 / 1 in fp32 | past exp's clamp
_BIAS = re.compile(r"(gru\d+_b|lstm\d+_b|ff1_b|ff2_b)$")


def saturated_biases(w, seed=77):
    """A copy of the model `w` with one of LEVELS added to every bias of its recurrent layers and feedforward2_tanh joins (matrices in
    sorted name order, one RandomState); no weight matrix changes, so every |w| stays far below the split products' operand limit."""
    w = dict(w)
    rng = np.random.RandomState(seed)
    for nm in sorted(w):
        if _BIAS.match(nm):
            w[nm] = (w[nm] + rng.choice(LEVELS, size=w[nm].shape)).astype(np.float32)
    return w


def bias_levels(plain, sat, name):
    """the level saturated_biases added to each entry of bias `name` (the plain biases lie within +-0.1)"""
    return np.rint(sat[name].astype(np.float64) - plain[name].astype(np.float64)).astype(np.int64)


# (model, size, model seed, samples or events).  Window 11, stride 5 meets the convolution's right-edge quirk iff N % 5 != 0, window 19 iff
# N % 5 == 0: every convolution gets one length of each kind; both give T = 200 blocks.
GRU_NETS = [("rgrgr_r94", 96), ("rgrgr_r10", 96), ("rnnrf_r94", 96), ("rnnrf_r94", 64), ("rnnrf_r94", 32)]
BI_NETS = [("raw_r94", 96), ("raw_r94", 32)]
EVENT_NETS = [("nanonet_events", 96), ("nanonet_events", 32)]
CASES = [(name, size, seed, n) for name, size in GRU_NETS + BI_NETS for seed, n in ((1, 1000), (11, 998))] + \
        [(name, size, seed, 200) for name, size in EVENT_NETS for seed in (1, 11)]
case_id = lambda c: "%s-%d-seed%d-%d" % c


@functools.lru_cache(maxsize=None)
def weights(name, size, seed):
    plain = model.synthetic_model(name, seed=seed, size=size)
    return plain, saturated_biases(plain)


@functools.lru_cache(maxsize=None)
def case_input(name, seed, n):
    """the read: a med/MAD-normalised signal, or the windowed float32 features [nevent][12] of an event read (the same array goes to every
    implementation: the studentisation's reciprocal square root is an estimate whose bits differ between CPUs, tests/test_net_f64.py)"""
    if name == "nanonet_events":
        import oracle
        f3 = oracle.window(oracle.features_from_events(synth.synthetic_events(n, 700 + seed), True), 3, 1)
        return np.ascontiguousarray(f3, dtype=np.float32)
    return synth.medmad_normalise(synth.synthetic_signal(n, 600 + seed))


def gru_gate_inputs(xaff, sW, sW2, out, backward):
    """[T][3S] gate pre-activations [z | r | candidate] of the steps that produced `out` = make_net_f64.gru(xaff, sW, sW2, backward)"""
    S = sW2.shape[0]
    hprev = np.zeros_like(out)
    if backward:
        hprev[:-1] = out[1:]
    else:
        hprev[1:] = out[:-1]
    g = xaff.copy()
    g[:, :2 * S] += hprev @ sW.T
    g[:, 2 * S:] += (F.logistic(g[:, S:2 * S]) * hprev) @ sW2.T
    return g


def lstm_with_gate_inputs(xaff, sW, p, backward):
    """make_net_f64.lstm, statement for statement, keeping what each activation is applied to: (out[T][S], pre[T][4S]) with pre =
    [input (tanh) | update | forget | output], the three logistic gates WITH their peephole terms (layers.c:811-825)"""
    T, S = xaff.shape[0], sW.shape[1]
    out, pre = np.zeros((T, S)), np.zeros((T, 4 * S))
    o, c = np.zeros(S), np.zeros(S)
    for t in (range(T - 1, -1, -1) if backward else range(T)):
        g = xaff[t] + sW @ o
        pf = g[2 * S:3 * S] + c * p[S:2 * S]
        pu = g[S:2 * S] + c * p[:S]
        forget = F.logistic(pf) * c
        update = F.logistic(pu) * F.tanh_ref(g[:S])
        c = forget + update
        po = g[3 * S:] + c * p[2 * S:]
        o = F.logistic(po) * F.tanh_ref(c)
        out[t] = o
        pre[t] = np.concatenate([g[:S], pu, pf, po])
    return out, pre


class Statement(object):
    """layers[upto]: float64 activations [T][units] as scrappie_hip_trunk / orc_trunk number them (0: the convolution, absent for events);
    out: log-posterior [T][NS], or the CRF transitions of rnnrf; gates: [(label, pre-activations)] of every recurrent layer and join"""

    def __init__(self, w, x, min_prob=1e-5):
        f64, arch = F.f64, w["arch"]
        self.arch, self.layers, self.gates = arch, {}, []
        if arch == "events":
            act = F.f64(x).reshape(-1, 12)            # what window3 makes of the features, handed in as float32
        else:
            act = F.convolution(f64(x), f64(w["conv_W"]), f64(w["conv_b"]), int(w["stride"]))
            act = F.elu(act) if w["conv_act"] == "elu" else F.tanh_ref(act)
            self.layers[0] = act
        if arch in ("rgrgr", "rnnrf"):
            for l in range(5):
                iW, sW, sW2, b = (f64(w["gru%d_%s" % (l, k)]) for k in ("iW", "sW", "sW2", "b"))
                xaff, back = act @ iW.T + b, l % 2 == 0
                out = F.gru(xaff, sW, sW2, backward=back)
                self.gates.append(("gru%d" % l, gru_gate_inputs(xaff, sW, sW2, out, back)))
                act = out + act if arch == "rnnrf" else out
                self.layers[l + 1] = act
        else:
            for lvl in range(2):
                hs = []
                for d in range(2):
                    l = 2 * lvl + d
                    if arch == "raw":
                        iW, sW, sW2, b = (f64(w["gru%d_%s" % (l, k)]) for k in ("iW", "sW", "sW2", "b"))
                        xaff = act @ iW.T + b
                        hs.append(F.gru(xaff, sW, sW2, backward=(d == 1)))
                        self.gates.append(("gru%d" % l, gru_gate_inputs(xaff, sW, sW2, hs[-1], d == 1)))
                    else:
                        iW, sW, b, p = (f64(w["lstm%d_%s" % (l, k)]) for k in ("iW", "sW", "b", "p"))
                        xaff = act @ iW.T + b
                        hs.append(F.lstm(xaff, sW, p, backward=(d == 1)))
                        mine, pre = lstm_with_gate_inputs(xaff, sW, p, d == 1)
                        assert np.array_equal(mine, hs[-1])         # the census looks at the gates of make_net_f64's own steps
                        self.gates.append(("lstm%d" % l, pre))
                k = "ff%d" % (lvl + 1)
                pre = hs[0] @ f64(w[k + "_Wf"]).T + hs[1] @ f64(w[k + "_Wb"]).T + f64(w[k + "_b"])
                self.gates.append((k, pre))
                act = F.tanh_ref(pre)
                self.layers[lvl + 1] = act
        if arch == "rnnrf":
            self.out = F.globalnorm(act, f64(w["ff_W"]), f64(w["ff_b"]))
        else:
            self.out = F.robustlog(F.softmax_temperature(act, f64(w["ff_W"]), f64(w["ff_b"]), 1.0, 1.0), min_prob)

    def census(self, labels=None):
        """share of the pre-activations (of the named layers; default all) in each of the five BANDS"""
        v = np.abs(np.concatenate([g.ravel() for nm, g in self.gates if labels is None or nm in labels]))
        return np.histogram(v, bins=BANDS)[0] / float(v.size)


@functools.lru_cache(maxsize=None)
def statement(case):
    """the float64 statement of a case of CASES on the saturated variant: computed once, shared by every test, never modified"""
    name, size, seed, n = case
    return Statement(weights(name, size, seed)[1], case_input(name, seed, n))


def compare(st, got_layers, got_out, who, scale=1.0):
    """got_layers {upto: float32 [T][units]} and got_out against the statement, at `scale` x the tolerances of tests/test_net_f64.py; prints
    and returns the measured maxima"""
    rep = {}
    for upto, got in sorted(got_layers.items()):
        want = st.layers[upto]
        assert got.shape == want.shape, (who, upto, got.shape, want.shape)
        assert np.all(np.isfinite(got)), (who, upto)
        rep["trunk%d" % upto] = float(np.max(np.abs(got.astype(np.float64) - want)))
    if got_out is not None:
        assert got_out.shape == st.out.shape and np.all(np.isfinite(got_out)), who
        have = got_out.astype(np.float64)
        if st.arch == "rnnrf":
            rep["dtrans"] = float(np.max(np.abs(have - st.out)))
        else:
            big = np.exp(st.out) > 1e-4
            rep["dp"] = float(np.max(np.abs(np.exp(have) - np.exp(st.out))))
            rep["dlogp"] = float(np.max(np.abs(have[big] - st.out[big])))
    print("%s: " % who + "  ".join("%s %.3g" % kv for kv in rep.items()))
    tol = {"dtrans": CRF_TOL, "dp": P_TOL, "dlogp": LOGP_TOL}
    for k, v in rep.items():
        assert v <= scale * tol.get(k, ACT_TOL), (who, k, v)
    return rep


def uptos(arch):
    return range(6) if arch in ("rgrgr", "rnnrf") else range(3) if arch == "raw" else range(1, 3)


# ------------------------------------------------------------------ the premise
def test_premise_plain_synthetic_weights_never_saturate():
    w = model.synthetic_model("rgrgr_r94", seed=1)
    st = Statement(w, case_input("rgrgr_r94", 1, 1000))
    for nm, g in st.gates:
        a = np.abs(g)
        print("%s: largest |pre-activation| %.2f, below 2: %.1f %%" % (nm, a.max(), 100.0 * np.mean(a < 2)))
    share = st.census()
    assert share[0] >= 0.97 and share[2] + share[3] + share[4] == 0, share


# ------------------------------------------------------------------ the census of the variant
@pytest.mark.parametrize("case", [c for c in CASES if c[0] not in ("raw_r94", "nanonet_events")], ids=case_id)
def test_census_gru_stack_every_band_populated(case):
    st = statement(case)
    share = st.census()
    print("%s: shares %s, largest %.1f" % (case_id(case), np.round(share, 3), max(np.abs(g).max() for _, g in st.gates)))
    assert np.all(share >= 0.10), share
    for nm, g in st.gates:                                  # and no layer is left out
        assert np.all(st.census({nm}) >= 0.10), (nm, st.census({nm}))


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("raw_r94", "nanonet_events")], ids=case_id)
def test_census_bigru_lstm_and_joins(case):
    """the bi-GRU's and the LSTM's layers (all four LSTM gates with their peephole terms) and the two feedforward2_tanh joins, each on its own"""
    st = statement(case)
    rec = "lstm%d" if case[0] == "nanonet_events" else "gru%d"
    assert [nm for nm, _ in st.gates] == [rec % 0, rec % 1, "ff1", rec % 2, rec % 3, "ff2"]
    joins = st.census({"ff1", "ff2"})                       # (a join of 32 units has 32 biases: the two are counted together)
    print("%s joins: shares %s" % (case_id(case), np.round(joins, 3)))
    assert joins[3] + joins[4] >= 0.10 and joins[0] >= 0.10, joins
    for nm, g in st.gates:
        share = st.census({nm})
        print("%s %s: shares %s, largest %.1f" % (case_id(case), nm, np.round(share, 3), np.abs(g).max()))
        if nm.startswith("ff"):
            continue
        assert share[3] + share[4] >= 0.10 and share[0] >= 0.10, (nm, share)
        if nm.startswith("lstm"):                           # each of the four gates
            S = g.shape[1] // 4
            for k, gate in enumerate(("input", "update", "forget", "output")):
                a = np.abs(g[:, k * S:(k + 1) * S])
                assert np.mean(a >= 17) >= 0.10 and np.mean(a < 2) >= 0.10, (nm, gate)


# ------------------------------------------------------------------ the reference alone
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_within_half_tolerance_of_float64(orc, case):
    name, size, seed, n = case
    w = weights(name, size, seed)[1]
    om, x, st = orc.OracleModel(w), case_input(name, seed, n), statement(case)
    if name == "nanonet_events":
        layers = {u: orc.events_trunk(om, x, u) for u in uptos(st.arch)}
        out = orc.events_posterior(om, x, min_prob=1e-5)
    else:
        layers = {u: orc.trunk(om, x, u) for u in uptos(st.arch)}
        out = orc.posterior(om, x, min_prob=1e-5)
    compare(st, layers, out, "oracle " + case_id(case), scale=0.5)
