"""The batched CRF posterior without a GPU: the library exports the new entry points, the planner of the output buffer
(scrappie_hip_crf_post_plan) keeps its promises, the float64 model the GPU tests use (tests/crf_post_model.py) agrees with the host's
posterior_crf -- itself pinned to the compiled reference -- on the five input families, and the planner, the staging of a launch's
matrices and the result container run clean under the address and undefined-behaviour sanitizers (tests/crf_post_asan.c, a program of
its own)."""
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa

import crf_post_model as cpm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_new_symbols():
    for name in ("scrappie_hip_crf_post_plan", "scrappie_hip_posterior_crf_batch", "scrappie_hip_basecall_batch_probs",
                 "scrappie_hip_crf_post_timing", "scrappie_hip_crf_post_launch_count"):
        assert hasattr(sa.lib(), name), name
    assert sa.lib().scrappie_hip_crf_post_launch_count() >= 0        # a host counter: no device is asked


def test_planner_aligned_starts_no_overlap():
    lens = [1, 0, 7, 8, 800, 3]
    off, total = sa.crf_post_plan(lens)
    assert len(off) == len(lens)
    spans = []
    for n, o in zip(lens, off):
        assert o % 4 == 0 and o >= 0, (n, o)                          # 16-byte starts
        if n:
            spans.append((int(o), int(o) + (n + 1) * 5))
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, "reads overlap"
    assert total >= spans[-1][1]                                      # the total covers the last read
    assert off[2] == off[1]                                           # the empty read takes no room
    assert total <= sum((n + 1) * 5 + 3 for n in lens if n)           # ... and nobody more than its floats and the alignment
    assert sa.crf_post_plan([]) [1] == 0
    assert sa.crf_post_plan([0, 0])[1] == 0


@pytest.mark.parametrize("name", cpm.FAMILIES)
def test_float64_model_against_host_posterior_crf(name):
    """e_ref of the GPU tests: the host function's maximum absolute error against the float64 model, per family -- finite, no NaN, and
    small against what a probability is (the bound the device gets is 4 e_ref + 1e-6)."""
    mats, want, e_ref, per_read = cpm.reference(name)
    assert e_ref == max(per_read) and len(per_read) == len(mats)
    assert sorted(len(m) for m in mats) == sorted(cpm.block_counts()) and len(mats) == cpm.NREAD
    for w, m in zip(want, mats):
        assert w.shape == (len(m) + 1, 5) and np.all(np.isfinite(w)) and np.all(w >= 0) and np.all(w <= 1)
        # Q16: the extra e^0 in every total.  A column sums to 1 - e^-total, and a total grows by about two a block: below one wherever a
        # float64 can tell (the short reads), one to rounding further out
        assert np.all(w.sum(axis=1) <= 1.0 + 1e-12)
        if len(m) <= 2 and name != "peaked":
            assert np.all(w.sum(axis=1) < 1.0)
    print("family %-9s host posterior_crf against float64: e_ref = %.3g, device bound %.3g" % (name, e_ref, cpm.bound(e_ref)))
    assert np.isfinite(e_ref)
    assert e_ref < 0.05, "the host function and the float64 model describe different recursions"


def test_host_side_under_sanitizers(tmp_path):
    """tests/crf_post_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the plan, the staging of matrices held in
    buffers of exactly their last column's 25th float into a buffer of exactly the size the staging reports, result matrices from a
    buffer of exactly the plan's total"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "crf_post_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "crf_post_asan.c"), os.path.join(csrc, "sh_host.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]
