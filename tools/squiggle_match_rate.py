#!/usr/bin/env python3
"""Rate of squiggle matching on the engine (scrappie_hip_squiggle_match_batch; a DESIGN.md record, not bench.py's `value`).
A few hundred simulated reads at mappy-like sizes -- the sample counts of the bundled reads (tests/golden/reads/reads.json)
with positions = samples / 8, a third of the reads at each size -- each mapped in Viterbi with its path to its own
simulated squiggle (synth.simulated_squiggle).  Reports the per-call time of the three stages, reads/s, DP cells/s, the
bytes/s of traceback written and the samples/s one workgroup sustains; beside it the reference's own time for a few of
the same reads (oracle/_ref/libref_decode.so, one thread), whose traceback is samples x states int32 per read.
usage: squiggle_match_rate.py [reads=300] [repeats=3] [reference_reads=2]"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import scrappie_amd as sa
from scrappie_amd import synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
nref = int(sys.argv[3]) if len(sys.argv) > 3 else 2
sizes = sorted(v["n"] for v in json.load(open(os.path.join(ROOT, "tests", "golden", "reads", "reads.json"))).values())
sigs, sqs = [], []
for i in range(n):
    ns = sizes[i % len(sizes)]
    params, sig, _ = synth.simulated_squiggle(ns // 8, 100 + i)
    if len(sig) < ns:
        sig = np.tile(sig, ns // len(sig) + 1)
    sigs.append(np.ascontiguousarray(sig[:ns]))
    sqs.append(params)
T = int(sa.lib().scrappie_hip_squiggle_lds_max_pos())
cells = float(sum(len(x) * (2 * len(p) + 2) for x, p in zip(sigs, sqs)))
samples = float(sum(len(x) for x in sigs))
tb_bytes = float(sum(len(x) * ((len(p) + 63) // 64) * 32 + len(x) * 4 for x, p in zip(sigs, sqs)))

eng = sa.Engine(0)
eng.match_squiggle(sigs[:6], sqs[:6], path=True)            # warm-up: buffers, kernels
walls, splits = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    res = eng.match_squiggle(sigs, sqs, viterbi=True, path=True)
    walls.append(time.perf_counter() - t0)
    splits.append(eng.squiggle_timing())
assert all(np.isfinite(s) and p is not None and len(p) == len(x) for (s, p), x in zip(res, sigs))
wall = min(walls)
sp = splits[int(np.argmin(walls))]
t0 = time.perf_counter()
fwd = eng.match_squiggle(sigs, sqs, viterbi=False)
wall_f = time.perf_counter() - t0
spf = eng.squiggle_timing()
assert all(np.isfinite(s) for s, _ in fwd)
# one read alone: what one workgroup sustains (samples are a serial chain)
big = int(np.argmax([len(x) for x in sigs]))
eng.match_squiggle([sigs[big]], [sqs[big]], path=True)
one = eng.squiggle_timing()

print("squiggle_match_rate: %d reads of %s samples, positions = samples / 8 (all above the %d positions whose rows fit LDS: rows in "
      "device scratch), Viterbi + path" % (n, "/".join(str(s) for s in sizes), T))
print("wall %.3f s (best of %d: %s) = %.1f reads/s, %.3e samples/s, %.3e DP cells/s (a cell: one state of one sample, 2 npos + 2 states)"
      % (wall, reps, ", ".join("%.3f" % w for w in walls), n / wall, samples / wall, cells / wall))
print("per call: tables + uploads %.1f ms, k_squig %.1f ms, k_squig_walk + results %.1f ms (host clock, stream drained between stages)"
      % (sp["tables_ms"], sp["match_ms"], sp["walk_ms"]))
print("k_squig alone: %.3e DP cells/s; traceback written %.2f GB = %.3e bytes/s over k_squig's time (4 bits per sample and position + END's int32 per sample)"
      % (cells / (sp["match_ms"] * 1e-3), tb_bytes / 1e9, tb_bytes / (sp["match_ms"] * 1e-3)))
print("one read alone (%d samples x %d positions): k_squig %.1f ms = %.3e samples/s per workgroup, walk + results %.1f ms"
      % (len(sigs[big]), len(sqs[big]), one["match_ms"], len(sigs[big]) / (one["match_ms"] * 1e-3), one["walk_ms"]))
print("forward scores, same reads: wall %.3f s, k_squig %.1f ms" % (wall_f, spf["match_ms"]))
eng.close()

from test_squiggle_cpu import PENS, call_squig, ref_squiggle_lib
R = ref_squiggle_lib()
if R is None or nref <= 0:
    print("reference: oracle/_ref/libref_decode.so not built -- not measured")
else:
    # the smallest size only: the reference's traceback is samples x (2 npos + 2) int32 -- 0.85 GB for it, 4.1 and 6.6 GB for the other two
    idx = [i for i in range(n) if len(sigs[i]) == sizes[0]][:nref]
    secs = []
    for i in idx:
        t0 = time.perf_counter()
        s, p = call_squig(R, sigs[i], 0, len(sigs[i]), sqs[i], PENS[0], True)
        secs.append(time.perf_counter() - t0)
        assert np.float32(res[i][0]).tobytes() == s.tobytes() and np.array_equal(res[i][1], p)
    c = float(len(sigs[idx[0]]) * (2 * len(sqs[idx[0]]) + 2))
    print("reference, one thread, %d reads of %d samples x %d positions (the smallest size; its traceback is %.2f GB per read): %s s per read = %.3e DP cells/s; "
          "scores and paths equal the GPU's" % (len(idx), len(sigs[idx[0]]), len(sqs[idx[0]]), c * 4 / 1e9, ", ".join("%.2f" % x for x in secs), c / min(secs)))
    print("at that rate the %d reads of this run take %.0f s on one reference thread" % (n, cells / (c / min(secs))))
