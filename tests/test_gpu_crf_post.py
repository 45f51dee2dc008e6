"""The batched CRF posterior on the GPU (run with -m gpu on an MI355X): k_crf_post (csrc/sh_crf_post.h) in both its forms -- on host
matrices (Engine.posterior_crf) and inside a launch group (Engine.basecall(..., base_probs=True)) -- against the float64 model of
tests/crf_post_model.py.

Bound, per input family: max |device - float64| <= 4 * e_ref + 1e-6, e_ref being the host posterior_crf's own maximum error on the same
family, computed here every run (crf_post_model.bound says why 4 and why the floor).  Measured ratios: profiles/crf_post_error.txt."""
import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth

import crf_post_model as cpm

pytestmark = pytest.mark.gpu


def sig(n, seed):
    return synth.medmad_normalise(synth.synthetic_signal(n, seed))


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    e.load_model("rnnrf_r94", model.synthetic_model("rnnrf_r94", seed=11, size=96))
    e.load_model("small", model.synthetic_model("rgrgr_r94", seed=12, size=32, nstate=65))      # a transducer: no base probabilities
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs():
    """family -> (matrices, float64 model, e_ref, e_ref of every read): computed once, shared, never changed"""
    return {name: cpm.reference(name) for name in cpm.FAMILIES}


@pytest.fixture(scope="module")
def dev(eng, refs):
    """family -> what one call of 33 reads returns, and how many launches of k_crf_post it took"""
    out = {}
    for name in cpm.FAMILIES:
        before = sa.lib().scrappie_hip_crf_post_launch_count()
        got = eng.posterior_crf(refs[name][0])
        out[name] = (got, sa.lib().scrappie_hip_crf_post_launch_count() - before)
    return out


@pytest.mark.parametrize("name", cpm.FAMILIES)
def test_family_within_four_host_errors(refs, dev, name):
    mats, want, e_ref, per_read = refs[name]
    got = dev[name][0]
    assert all(g is not None and g.shape == (len(m) + 1, 5) and g.dtype == np.float32 for g, m in zip(got, mats))
    assert all(np.all(np.isfinite(g)) for g in got), "NaN or infinity"
    err = cpm.max_err(got, want)
    print("family %-9s device error %.3g, e_ref %.3g, ratio %.4f, bound %.3g" % (name, err, e_ref, err / max(e_ref, 1e-30), cpm.bound(e_ref)))
    assert err <= cpm.bound(e_ref)
    # the family's maximum sits in its one read of 800 blocks (messages of magnitude 2 T, ulps of 1e-4): the same bound read by read, each against
    # the host's error on that read, so that the short reads -- the ring's and the tile's edges -- are held to what a short read allows
    worst = 0.0
    for g, w, m, e_r in zip(got, want, mats, per_read):
        err_r = cpm.max_err([g], [w])
        worst = max(worst, (err_r - 1e-6) / max(e_r, 1e-30))
        assert err_r <= cpm.bound(e_r), (len(m), err_r, e_r)
    print("family %-9s read by read: largest (device error - 1e-6) / e_ref of the read = %.3f" % (name, worst))


def test_structure_of_a_posterior(refs, dev):
    mats, want, e_ref, _ = refs["normal"]
    for g, w, m in zip(dev["normal"][0], want, mats):
        assert g.shape == (len(m) + 1, 5)
        assert np.all(g >= 0.0) and np.all(g <= 1.0)
        s = g.astype(np.float64).sum(axis=1)
        # Q16: a column sums to 1 - e^-total.  Below one wherever float32 can tell (a read of a block or two).  Further out the total grows by
        # about two a block, the exact sum is one to 1e-17, and what a float32 recursion returns -- the host's as much as the device's -- is one
        # to the error of its five terms (messages of magnitude 2 T carry ulps of 1e-4 at 800 blocks): held to the model's sum by the families' bound
        if len(m) <= 2:
            assert np.all(s < 1.0)
        assert np.max(np.abs(s - w.sum(axis=1))) <= cpm.bound(e_ref)
        assert np.all(s <= 1.0 + cpm.bound(e_ref))


def test_one_launch_for_33_reads(dev):
    assert [dev[name][1] for name in cpm.FAMILIES] == [1] * len(cpm.FAMILIES)


def test_ragged_tile_reads_alone_bit_identical(eng, refs, dev):
    """a lane that read or wrote across its read's end in the tile would show here: every read alone (a tile of one) gives the array it got
    among 32 others"""
    mats = refs["normal"][0]
    for k, m in enumerate(mats):
        alone = eng.posterior_crf([m])[0]
        assert np.array_equal(alone, dev["normal"][0][k]), (k, len(m))


def test_base_probs_in_the_pipeline(eng):
    rng = np.random.default_rng(3)
    min_n = eng.min_samples("rnnrf_r94")
    lens = [int(x) for x in rng.integers(300, 1501, 40)]
    sigs = [sig(n, 7000 + i) for i, n in enumerate(lens)]
    sigs.insert(5, sig(min_n - 1, 7100)); sigs.insert(30, sig(5, 7101))
    p = eng.default_params()
    plain = eng.basecall(sigs, "rnnrf_r94", p)
    probs = eng.basecall(sigs, "rnnrf_r94", p, base_probs=True)
    assert [c is None for c in plain] == [c is None for c in probs] == [i in (5, 30) for i in range(len(sigs))]
    for a, b in zip(plain, probs):
        if a is None:
            continue
        assert (a["bases"], a["nblock"]) == (b["bases"], b["nblock"])
        assert np.float32(a["score"]).tobytes() == np.float32(b["score"]).tobytes()
        assert b["base_probs"].shape == (b["nblock"] + 1, 5) and b["base_probs"].dtype == np.float32
    # both forms of the kernel run the same recursion on the same floats
    for i in (0, 17, 41):
        trans = eng.posterior(sigs[i], "rnnrf_r94", min_prob=p.min_prob, tempW=p.tempW, tempb=p.tempb)
        assert np.array_equal(probs[i]["base_probs"], eng.posterior_crf([trans])[0]), i
        want = cpm.model_f64([trans])
        e_ref = cpm.max_err([cpm.host_posterior(trans)], want)
        err = cpm.max_err([probs[i]["base_probs"]], want)
        print("read %d (%d blocks): device error %.3g, e_ref %.3g" % (i, len(trans), err, e_ref))
        assert err <= cpm.bound(e_ref)


def test_slot_discipline_three_launch_groups(eng):
    """per-slot buffers, the engine's shared transitions and the copy stream: a call cut into four launch groups gives every read the array
    it gets alone"""
    rng = np.random.default_rng(4)
    sigs = [sig(int(n), 7200 + i) for i, n in enumerate(rng.integers(300, 701, 100))]
    eng.set_max_launch_reads(32)
    try:
        together = eng.basecall(sigs, "rnnrf_r94", base_probs=True)
    finally:
        eng.set_max_launch_reads(16384)
    for k, s in enumerate(sigs):
        alone = eng.basecall([s], "rnnrf_r94", base_probs=True)[0]
        assert together[k]["bases"] == alone["bases"], k
        assert np.array_equal(together[k]["base_probs"], alone["base_probs"]), k


def test_wrong_model_and_bad_input(eng, refs, dev):
    with pytest.raises(ValueError):
        eng.basecall([sig(600, 1)], "small", base_probs=True)
    mats = refs["normal"][0]
    got = eng.posterior_crf([mats[0], np.zeros((7, 24), np.float32), mats[1], np.zeros((0, 25), np.float32)])
    assert got[1] is None and got[3] is None
    assert np.array_equal(got[0], dev["normal"][0][0]) and np.array_equal(got[2], dev["normal"][0][1])
