#!/usr/bin/env python3
"""Rate of banded squiggle matching on the engine (scrappie_hip_squiggle_match_banded_batch, sh_squig_band.h; a DESIGN.md
record, not bench.py's `value`).  The reads of tools/squiggle_match_rate.py -- simulated reads with the sample counts of the
bundled reads and positions = samples / 8, each mapped in Viterbi with its path to its own simulated squiggle -- once without
a band (k_squig, as that tool measures it) and then inside the diagonal band of half-widths 128, 512 and 2048 positions
(k_squig_band).  Per setting: the call's wall time, the three stages of squiggle_timing, DP cells/s over the kernel's time (a
cell: one state of one sample inside the band, 2 width + 2 per sample), the traceback bytes, and how many reads get the
unbanded score and path (a band that misses the best path gives another, lower-scoring one).  Then the longest read alone.
usage: squiggle_band_rate.py [reads=300] [repeats=3] [halfwidths=128,512,2048]"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scrappie_amd as sa
from scrappie_amd import synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
halfwidths = [int(h) for h in (sys.argv[3] if len(sys.argv) > 3 else "128,512,2048").split(",")]
sizes = sorted(v["n"] for v in json.load(open(os.path.join(ROOT, "tests", "golden", "reads", "reads.json"))).values())
sigs, sqs = [], []
for i in range(n):
    ns = sizes[i % len(sizes)]
    params, sig, _ = synth.simulated_squiggle(ns // 8, 100 + i)
    if len(sig) < ns:
        sig = np.tile(sig, ns // len(sig) + 1)
    sigs.append(np.ascontiguousarray(sig[:ns]))
    sqs.append(params)
samples = float(sum(len(x) for x in sigs))
big = int(np.argmax([len(x) for x in sigs]))
M = int(sa.lib().scrappie_hip_squiggle_band_lds_max_width())


def measure(eng, S, Q, band):
    """best of `reps` calls: (wall s, all walls, the stages of the best call, its results, band launches by form)"""
    walls, splits, res = [], [], None
    f0 = sa.squiggle_band_form_counts()
    for _ in range(reps):
        t0 = time.perf_counter()
        res = eng.match_squiggle(S, Q, viterbi=True, path=True, band=band)
        walls.append(time.perf_counter() - t0)
        splits.append(eng.squiggle_timing())
    f1 = sa.squiggle_band_form_counts()
    return min(walls), walls, splits[int(np.argmin(walls))], res, {k: f1[k] - f0[k] for k in f1}


def line(tag, S, Q, width, wall, walls, sp, kernel):
    """one setting: width None = unbanded (cells 2 npos + 2 per sample, traceback over npos)"""
    wd = [len(q) if width is None else min(width, len(q)) for q in Q]
    cells = float(sum(len(x) * (2 * w + 2) for x, w in zip(S, wd)))
    tb = float(sum(len(x) * ((w + 63) // 64) * 32 + len(x) * 4 for x, w in zip(S, wd)))
    print("%s: wall %.3f s (best of %d: %s); tables + uploads %.1f ms, %s %.1f ms, walk + results %.1f ms; %.3e DP cells, %.3e cells/s and "
          "%.3e samples/s over the kernel's time; traceback %.3f GB"
          % (tag, wall, len(walls), ", ".join("%.3f" % w for w in walls), sp["tables_ms"], kernel, sp["match_ms"], sp["walk_ms"], cells,
             cells / (sp["match_ms"] * 1e-3), sum(len(x) for x in S) / (sp["match_ms"] * 1e-3), tb / 1e9))


eng = sa.Engine(0)
eng.match_squiggle(sigs[:6], sqs[:6], path=True)                     # warm-up: buffers, both kernels
eng.match_squiggle(sigs[:6], sqs[:6], path=True, band=halfwidths[0])
print("squiggle_band_rate: %d reads of %s samples, positions = samples / 8, Viterbi + path; bands up to %d positions wide keep their rows in LDS"
      % (n, "/".join(str(s) for s in sizes), M))
wall, walls, sp, plain, _ = measure(eng, sigs, sqs, None)
assert all(np.isfinite(s) and p is not None for s, p in plain)
line("unbanded", sigs, sqs, None, wall, walls, sp, "k_squig")
for h in halfwidths:
    width = 2 * h + 1
    wall, walls, sp, res, forms = measure(eng, sigs, sqs, h)
    same = sum(1 for (s, p), (s0, p0) in zip(res, plain) if p is not None and np.float32(s).tobytes() == np.float32(s0).tobytes() and np.array_equal(p, p0))
    nopath = sum(1 for s, p in res if not np.isfinite(s))
    line("band h = %d (width %d, %s home)" % (h, width, "LDS" if width <= M else "scratch"), sigs, sqs, width, wall, walls, sp, "k_squig_band")
    print("    %d of %d reads get the unbanded score and path, %d have no path inside the band; k_squig_band launches (viterbi, scratch): %r"
          % (same, n, nopath, sorted(forms.items())))
print("the longest read alone (%d samples x %d positions): what one workgroup sustains" % (len(sigs[big]), len(sqs[big])))
S, Q = [sigs[big]], [sqs[big]]
wall, walls, sp, one, _ = measure(eng, S, Q, None)
line("  unbanded", S, Q, None, wall, walls, sp, "k_squig")
for h in halfwidths:
    wall, walls, sp, res, _ = measure(eng, S, Q, h)
    line("  band h = %d" % h, S, Q, 2 * h + 1, wall, walls, sp, "k_squig_band")
    print("    score %r (unbanded %r), path %s" % (res[0][0], one[0][0], "equal" if res[0][1] is not None and np.array_equal(res[0][1], one[0][1]) else "differs"))
eng.close()
