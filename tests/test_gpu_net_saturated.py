"""The recurrent layers past saturation on the device (run with -m gpu on an MI355X), through the C ABI.

The networks: tests/test_net_saturated_cpu.py's variant of the synthetic models (a level of 0, +-4, +-10, +-30 or +-120 added to every bias of
the recurrent layers and joins: a fifth of the gates each linear, bending, saturated, exactly 0 / 1 in fp32, and past the clamp of the
exponential) against the float64 statement of every layer, at the tolerances of tests/test_net_f64.py -- the same module shows that oracle.c
stays within half of them on these very cases.  Every kernel form of the layers: the split products (k_gru_proj, k_lstm_proj), the exact-fp32
fallback (k_affine<F32> + k_gru_lanes, debug option force_f32_layers), the two-kernel LSTM (k_affine + k_lstm_lanes, SH_GRU_SEPARATE=1 in a
process of its own), one and two tiles per workgroup on a ragged batch; and a state that must be held bit for bit: a unit whose update gate is
exactly 1.0f stays at the 0.0f it started from.

The activation forms on their own (scrappie_hip_debug_gates): a network tolerance of 1e-5 cannot see two ulps of an activation, so the ten
forms of sh_kernels.h run on a million values that weights do not reach -- +-130, the clamp +-88.3762626647949 and its neighbours, signed
zeros, subnormals, 1e-8 .. 1e-3 -- and are held to each other bit for bit where the source says they are the same operations, and to float64.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import make_net_f64 as F
import scrappie_amd as sa
from scrappie_amd import model, synth

from test_gpu_parity import P_TOL, LOGP_TOL, CRF_TOL
import test_net_saturated_cpu as sat
from test_net_saturated_cpu import CASES, case_id, case_input, compare, statement, uptos, weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


def _load(eng, case, exact=False):
    """the saturated model of a case under a name of its own, on the split kernels or (exact) on the exact-fp32 kernels"""
    name, size, seed, n = case
    key = "sat_%s_%d_%d%s" % (name, size, seed, "_f32" if exact else "")
    if key not in eng._models:
        try:
            eng.debug_option("force_f32_layers", 1 if exact else 0)
            eng.load_model(key, weights(name, size, seed)[1])
        finally:
            eng.debug_option("force_f32_layers", 0)
    return key


def _run(eng, key, case):
    x = case_input(case[0], case[2], case[3]).ravel()
    st = statement(case)
    return {u: eng.trunk(x, key, u) for u in uptos(st.arch)}, eng.posterior(x, key, min_prob=1e-5)


# ------------------------------------------------------------------ every layer and the output against float64
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_split_kernels_per_layer_and_output_vs_float64(eng, case):
    layers, out = _run(eng, _load(eng, case), case)
    compare(statement(case), layers, out, "HIP split " + case_id(case))


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == 96 and c[0] != "nanonet_events"], ids=case_id)
def test_exact_fp32_kernels_per_layer_and_output_vs_float64(eng, case):
    st = statement(case)
    layers, out = _run(eng, _load(eng, case, exact=True), case)
    compare(st, layers, out, "HIP exact-fp32 " + case_id(case))
    # ... and the two forms against each other
    split = eng.posterior(case_input(case[0], case[2], case[3]), _load(eng, case), min_prob=1e-5)
    a, b = out.astype(np.float64), split.astype(np.float64)
    if st.arch == "rnnrf":
        d = float(np.max(np.abs(a - b)))
        print("  exact-fp32 against split: max |dtrans| %.3g" % d)
        assert d <= CRF_TOL
    else:
        big = np.exp(b) > 1e-4
        dp, dl = float(np.max(np.abs(np.exp(a) - np.exp(b)))), float(np.max(np.abs(a[big] - b[big])))
        print("  exact-fp32 against split: max |dp| %.3g, max |dlogp| %.3g" % (dp, dl))
        assert dp <= P_TOL and dl <= LOGP_TOL


def test_two_kernel_lstm_form_vs_float64_and_one_kernel_form(eng, tmp_path):
    """k_affine + k_lstm_lanes (SH_GRU_SEPARATE=1, a process of its own) on the saturated events model: against float64 at the full
    tolerances, and against k_lstm_proj to a tenth of the posterior's, as test_events_one_kernel_layer_vs_two_kernel_form holds them"""
    case = ("nanonet_events", 96, 1, 200)
    mpath, xpath, opath = str(tmp_path / "ev.scrm"), str(tmp_path / "f3.npy"), str(tmp_path / "two.npz")
    model.save_model(weights(*case[:3])[1], mpath)
    f3 = case_input(case[0], case[2], case[3])
    np.save(xpath, f3)
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
import scrappie_amd as sa
e = sa.Engine(0); e.load_model("nanonet_events", %r)
f3 = np.load(%r).ravel()
np.savez(%r, post=e.posterior(f3, "nanonet_events", min_prob=1e-5), t1=e.trunk(f3, "nanonet_events", 1), t2=e.trunk(f3, "nanonet_events", 2))
e.close()
""" % (ROOT, mpath, xpath, opath)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SH_GRU_SEPARATE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    two = np.load(opath)
    compare(statement(case), {1: two["t1"], 2: two["t2"]}, two["post"], "HIP two-kernel LSTM " + case_id(case))
    one = eng.posterior(f3.ravel(), _load(eng, case), min_prob=1e-5)
    assert one.shape == two["post"].shape
    d = float(np.max(np.abs(np.exp(one.astype(np.float64)) - np.exp(two["post"].astype(np.float64)))))
    print("  two-kernel against one-kernel form: max |dp| %.3g" % d)
    assert d <= P_TOL / 10


# ------------------------------------------------------------------ a state held exactly
def test_update_gate_of_exactly_one_holds_the_state_bit_for_bit(eng):
    """z = logistic(pre) is exactly 1.0f once pre > 17 (1 + e == 1 in fp32), and h = z h + (1 - z) hbar then keeps the zero initial state
    through all 200 blocks whatever the candidate is: not 1e-9, 0.0f.  First layer of rgrgr_r94, both kernel forms."""
    case = ("rgrgr_r94", 96, 1, 1000)
    plain, w = weights(*case[:3])
    S = 96
    level = sat.bias_levels(plain, w, "gru0_b")[:S]                 # the z block (layers.c:511)
    held = np.flatnonzero((level == 30) | (level == 120))
    assert len(held) >= 10
    st = statement(case)
    nm, g = st.gates[0]
    assert nm == "gru0" and g.shape == (200, 3 * S)
    assert np.all(g[:, held] > 17), float(g[:, held].min())         # the premise, from the float64 census: at every block
    assert np.all(st.layers[1][:, held] < 1e-7)
    x = case_input(case[0], case[2], case[3])
    for exact in (False, True):
        got = eng.trunk(x, _load(eng, case, exact=exact), 1)
        assert got.shape == (200, S)
        bad = np.flatnonzero(got[:, held].view(np.uint32) & 0x7FFFFFFF)
        print("%s: %d units with z = 1 over 200 blocks, %d values not zero (largest %.3g)" %
              ("exact-fp32" if exact else "split", len(held), len(bad), float(np.max(np.abs(got[:, held])))))
        assert len(bad) == 0


# ------------------------------------------------------------------ batch forms
def _decode(orc, post, p):
    sc, seq = orc.decode_transducer(post, p.stay_pen, p.skip_pen, p.local_pen, False)
    rc, seq = orc.homopolymer_path(post, seq)
    bases, pos = orc.overlapper(seq, 1024)
    return sc, bases, pos


def _posterior_vs_float64(w, x, post, who):
    st = sat.Statement(w, x)
    return compare(st, {}, post, who)


def test_ragged_batch_one_and_two_tiles_per_workgroup(eng, orc):
    case = ("rgrgr_r94", 96, 11, 998)
    key, w = _load(eng, case), weights(*case[:3])[1]
    lens = [400 + (i * 131) % 401 for i in range(32)]                  # 400 .. 800 samples, no two tiles alike
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 9100 + i)) for i, n in enumerate(lens)]
    p = eng.default_params(want_pos=1, local_pen=120.0)
    calls = {}
    try:
        for tiles in (2, 1):
            eng.debug_option("gru_tiles", tiles)
            calls[tiles] = eng.basecall(sigs, key, p)
            assert int(eng.debug_fetch("gru_tiles", np.int32)[0]) == tiles
    finally:
        eng.debug_option("gru_tiles", 0)
    for i, x in enumerate(sigs):
        post = eng.posterior(x, key, min_prob=p.min_prob)
        sc, bases, pos = _decode(orc, post, p)
        for tiles in (2, 1):
            c = calls[tiles][i]
            assert c is not None and c["nblock"] == post.shape[0], (tiles, i)
            assert c["bases"] == bases and np.float32(c["score"]) == np.float32(sc) and list(c["pos"]) == list(pos), (tiles, i)
        if i % 8 == 3:                                                  # four of them against float64 (min_prob as the statement's)
            _posterior_vs_float64(w, x, eng.posterior(x, key, min_prob=1e-5), "HIP split, read %d of the batch (%d samples)" % (i, lens[i]))


def test_ragged_event_batch(eng, orc):
    case = ("nanonet_events", 96, 11, 200)
    key, w = _load(eng, case), weights(*case[:3])[1]
    reads = [np.ascontiguousarray(orc.window(orc.features_from_events(synth.synthetic_events(n, 9200 + i), True), 3, 1), dtype=np.float32)
             for i, n in enumerate((300, 133, 64, 257, 17, 190))]
    p = eng.default_params(want_pos=1)
    calls = eng.basecall([r.ravel() for r in reads], key, p)
    for i, (r, c) in enumerate(zip(reads, calls)):
        post = eng.posterior(r.ravel(), key, min_prob=p.min_prob)
        sc, bases, pos = _decode(orc, post, p)
        assert c is not None and c["nblock"] == len(r), i
        assert c["bases"] == bases and np.float32(c["score"]) == np.float32(sc) and list(c["pos"]) == list(pos), i
        _posterior_vs_float64(w, r, eng.posterior(r.ravel(), key, min_prob=1e-5), "HIP events, read %d of the batch (%d events)" % (i, len(r)))


# ------------------------------------------------------------------ the activation forms on their own
CLAMP = 88.3762626647949            # sse_mathfun.h:215, as sh_kernels.h writes it
TINY = 1.2e-38                      # what a clamped and a clamp-free form may differ by past the clamp (sh_kernels.h, at d_logistic4_acc)
FLT_MIN = float(np.finfo(np.float32).tiny)
# Bounds against float64: twice the maximum measured on an MI355X over gate_inputs(), rounded up to one significant digit, and never above the
# caps: 1e-6 absolute for logistic / tanh, 4e-6 relative for exp.  Measured (every form of a function gives the same figure): logistic 1.02e-7
# absolute, 3.87e-6 relative below 0.5; tanh 2.0e-7; exp 3.84e-6 relative; elu 6.71e-8 absolute, 1.0 relative.  exp's figure is its argument's
# rounding, not v_exp_f32's: x log2(e) is rounded to fp32 at magnitudes up to 127.5 (half an ulp: 3.8e-6 of the exponent, 2.6e-6 of the result),
# with an fp32 log2(e) that is 1.3e-8 relative off (1.2e-6 of the result at |x| = 88); twice it would pass the cap, so the cap is the bound.
# DESIGN.md section 6 lists measured against asserted.
LOGISTIC_ABS, TANH_ABS = 3e-7, 4e-7
LOGISTIC_REL, EXP_REL = 8e-6, 4e-6
ELU_ABS, ELU_REL = 2e-7, 2.0


@pytest.fixture(scope="module")
def gate_inputs():
    f32 = np.float32
    rng = np.random.default_rng(20240917)
    c = f32(CLAMP)
    edge = np.array([c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(0)), 0.0, 17.4, 9.1, 88.4, 88.0, 87.0, 44.0, 44.25, 20.0], dtype=f32)
    sub = np.concatenate([np.array([1, 2, 3, 0x1234, 0x3FFFFF, 0x400000, 0x7FFFFF, 0x800000], dtype=np.uint32),
                          rng.integers(1, 0x800000, 1000).astype(np.uint32)]).view(f32)
    small = np.logspace(-8, -3, 50000).astype(f32)
    special = np.concatenate([edge, sub, small])
    parts = [special, -special]
    for a in (20.0, 100.0, 130.0):
        parts.append(rng.uniform(-a, a, 300001).astype(f32))
    x = np.concatenate(parts)
    assert np.all(np.isfinite(x)) and len(x) % 4 != 0                  # the last group of four is padded, not read past
    return x


@pytest.fixture(scope="module")
def gates(eng, gate_inputs):
    """every form on the whole set, once (d_exp_acc_inrange where it is defined: |x| < 88)"""
    x = gate_inputs
    out = {}
    for nm in sa.Engine.GATE_FORMS:
        if nm == "d_exp_acc_inrange":
            out[nm] = eng.debug_gates(nm, x[np.abs(x) < 88])
        else:
            out[nm] = eng.debug_gates(nm, x)
        assert np.all(np.isfinite(out[nm])), nm                        # no NaN, no inf, in any form
    return out


def _same_bits(a, b, x, what):
    bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
    print("%s: %d of %d differ" % (what, len(bad), len(a)))
    for i in bad[:8]:
        print("  x = %r: %r (%#010x) against %r (%#010x)" % (float(x[i]), float(a[i]), int(a[i:i + 1].view(np.uint32)[0]), float(b[i]), int(b[i:i + 1].view(np.uint32)[0])))
    assert len(bad) == 0, what


def test_gate_forms_scalar_and_vector_forms_same_bits(gate_inputs, gates):
    _same_bits(gates["d_tanh"], gates["d_tanh4"], gate_inputs, "d_tanh against d_tanh4")
    _same_bits(gates["d_logistic"], gates["d_logistic4"], gate_inputs, "d_logistic against d_logistic4")


def test_gate_forms_accumulator_forms_same_bits(eng, gate_inputs, gates):
    x = gate_inputs
    m = np.abs(x) <= 88
    _same_bits(gates["d_logistic4_acc"][m], gates["d_logistic4"][m], x[m], "d_logistic4_acc against d_logistic4, |x| <= 88")
    _same_bits(gates["d_tanh4_acc"][m], gates["d_tanh4"][m], x[m], "d_tanh4_acc against d_tanh4, |x| <= 88")
    _same_bits(gates["d_exp_acc"], gates["d_exp"], x, "d_exp_acc against d_exp")
    r = np.abs(x) < 88
    _same_bits(gates["d_exp_acc_inrange"], gates["d_exp"][r], x[r], "d_exp_acc_inrange against d_exp, |x| < 88")
    # past the clamp the clamped and the clamp-free forms part ways, by no more than 1.2e-38
    for a, b in (("d_logistic4_acc", "d_logistic4"), ("d_tanh4_acc", "d_tanh4")):
        d = float(np.max(np.abs(gates[a][~m].astype(np.float64) - gates[b][~m].astype(np.float64))))
        print("%s against %s, |x| > 88: max |difference| %.3g over %d values" % (a, b, d, int((~m).sum())))
        assert d <= TINY
    # a length that is no multiple of four, and a short one
    assert np.array_equal(eng.debug_gates("d_tanh4_acc", x[:13]).view(np.uint32), gates["d_tanh4_acc"][:13].view(np.uint32))


def _errors(got, want):
    """(max absolute error, max error relative to the float64 value where fp32 holds that value as a normal number, max absolute error below).
    The line is drawn at twice the smallest normal number: a result that rounds to just under it may be flushed like a subnormal."""
    g, err = got.astype(np.float64), np.abs(got.astype(np.float64) - want)
    normal = np.abs(want) >= 2 * FLT_MIN
    rel = float(np.max(err[normal] / np.abs(want[normal]))) if normal.any() else 0.0
    below = float(np.max(err[~normal])) if (~normal).any() else 0.0
    assert np.all(np.isfinite(g))
    return float(np.max(err)), rel, below


def test_gate_forms_vs_float64(gate_inputs, gates):
    """the reference's algebraic forms in float64 (make_net_f64: logistic, tanh_ref = 2 logistic(2x) - 1, elu, exp with its clamp).  tanh in
    absolute error only (the form cancels near 0); logistic below 0.5 and exp in relative error too, where the float64 value is a normal fp32
    number with room to spare (x > -86.6: _errors) -- below that fp32 has no relative precision to hold, v_exp_f32 and v_rcp_f32 flush, and the
    result is within 1.2e-38 of it."""
    x = gate_inputs
    x64 = x.astype(np.float64)
    rep = []
    for nm in ("d_logistic", "d_logistic4", "d_logistic4_acc"):
        want = F.logistic(x64)
        a, _, _ = _errors(gates[nm], want)
        neg = x64 < 0
        _, rel, below = _errors(gates[nm][neg], want[neg])
        rep.append("%s: max abs %.3g; below 0.5: max rel %.3g, max abs under FLT_MIN %.3g" % (nm, a, rel, below))
        print(rep[-1])
        assert a <= LOGISTIC_ABS and rel <= LOGISTIC_REL and below <= TINY, rep[-1]
    for nm in ("d_tanh", "d_tanh4", "d_tanh4_acc"):
        a, _, _ = _errors(gates[nm], F.tanh_ref(x64))
        print("%s: max abs %.3g" % (nm, a))
        assert a <= TANH_ABS, (nm, a)
    for nm in ("d_exp", "d_exp_acc", "d_exp_acc_inrange"):
        m = np.abs(x) < 88 if nm == "d_exp_acc_inrange" else np.ones(len(x), bool)
        _, rel, below = _errors(gates[nm], F.ref_exp(x64[m]))
        print("%s: max rel %.3g, max abs under FLT_MIN %.3g" % (nm, rel, below))
        assert rel <= EXP_REL and below <= TINY, (nm, rel, below)
    # elu = exp(x) - 1 below 0 cancels as the reference's own fp32 form does (util.h:190-198): an absolute error of an ulp of 1, which is
    # all of a result below 6e-8 -- the relative error says that and no more; the absolute one is the sharp figure
    want = F.elu(x64)
    a, rel, below = _errors(gates["d_elu"], want)
    print("d_elu: max abs %.3g, max rel %.3g, max abs under FLT_MIN %.3g" % (a, rel, below))
    assert np.array_equal(gates["d_elu"][x >= 0].view(np.uint32), x[x >= 0].view(np.uint32))          # the identity, -0 included
    assert a <= ELU_ABS and rel <= ELU_REL and below <= TINY, (a, rel, below)


def test_gate_forms_exact_saturation(gate_inputs, gates):
    """2^-25 < e: logistic(x) is exactly 1 from x = 17.4 on and tanh(x) exactly +-1 from |x| = 9.1 on; logistic(x) is 0 or below 1.2e-38
    for x <= -88.4 -- in every form, clamped or not"""
    x = gate_inputs
    for nm in ("d_logistic", "d_logistic4", "d_logistic4_acc"):
        y = gates[nm]
        assert np.all(y[x >= np.float32(17.4)] == 1.0), nm
        lo = y[x <= np.float32(-88.4)]
        assert len(lo) > 1000 and np.all(lo >= 0) and np.all(lo <= TINY), (nm, float(lo.max()))
        assert np.all((y >= 0) & (y <= 1)), nm
    for nm in ("d_tanh", "d_tanh4", "d_tanh4_acc"):
        y = gates[nm]
        assert np.all(y[x >= np.float32(9.1)] == 1.0) and np.all(y[x <= np.float32(-9.1)] == -1.0), nm
        assert np.all(np.abs(y) <= 1), nm
