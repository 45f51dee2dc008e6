#!/usr/bin/env python3
"""Rate of squiggle prediction on the engine (scrappie_hip_squiggle_predict_batch, k_sqnet; a DESIGN.md record, not
bench.py's `value`).  Two shapes: one sequence of 1 Mb, and 10 000 sequences of 400 bases, random bases, synthetic
squiggle_r94 weights (window 9).  Reports bases/s by wall clock and by k_sqnet's own time with the three stages of a
call, beside two comparisons: the CPU oracle composition (tests/test_sqnet_cpu.py ref32, one thread) on a shorter
sequence, and the fraction of the fp32 vector roof that 77 184 FLOP per base stand for.  Writes
profiles/sqnet_rate.txt.
usage: sqnet_rate.py [repeats=3] [oracle_bases=20000]"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import scrappie_amd as sa
from scrappie_amd import model

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
norc = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
FLOP_PER_BASE = 2 * (27 * 32 + 4 * 288 * 32 + 288 * 3)       # 77 184 at WL 9
ROOF = 157.3e12                                              # MI355X peak fp32 vector FLOP/s (256 CUs x 128 lanes x 2 x 2.4 GHz)

w = model.synthetic_model("squiggle_r94", seed=1)
eng = sa.Engine(0)
eng.load_model("squiggle_r94", w)
rng = np.random.RandomState(3)
shapes = [("one sequence of 1 Mb", [rng.randint(0, 4, size=1000000).astype(np.int32)]),
          ("10 000 sequences of 400 bases", [rng.randint(0, 4, size=400).astype(np.int32) for _ in range(10000)])]
eng.predict_squiggle([shapes[1][1][0]])                     # warm-up: buffers, the kernel's code object
lines = ["sqnet_rate: squiggle_r94 (window 9, synthetic weights), tile %d positions, %d FLOP per base" % (sa.lib().scrappie_hip_sqnet_tile(), FLOP_PER_BASE)]
for label, seqs in shapes:
    nb = float(sum(len(s) for s in seqs))
    walls, splits = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = eng.predict_squiggle(seqs)
        walls.append(time.perf_counter() - t0)
        splits.append(eng.sqnet_timing())
    assert all(o is not None and o.shape == (len(s), 3) and np.all(np.isfinite(o)) for o, s in zip(out, seqs))
    k = int(np.argmin(walls))
    sp = splits[k]
    knl = nb / (sp["net_ms"] * 1e-3)
    lines.append("%s: wall %.4f s (best of %d, Python list handling included) = %.3e bases/s; staging + upload %.2f ms, k_sqnet %.2f ms, "
                 "download + transform %.2f ms; k_sqnet alone %.3e bases/s = %.2f TFLOP/s = %.1f%% of the %.1f TFLOP/s fp32 vector roof"
                 % (label, walls[k], reps, nb / walls[k], sp["upload_ms"], sp["net_ms"], sp["download_ms"], knl, knl * FLOP_PER_BASE / 1e12,
                    100.0 * knl * FLOP_PER_BASE / ROOF, ROOF / 1e12))
eng.close()

from test_sqnet_cpu import ref32
codes = rng.randint(0, 4, size=norc).astype(np.int32)
t0 = time.perf_counter()
ref32(w, codes)
dt = time.perf_counter() - t0
lines.append("CPU oracle composition (orc_convolution + orc_tanh_activation_inplace + numpy residual, one thread), %d bases: %.3f s = %.3e bases/s"
             % (norc, dt, norc / dt))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
open(os.path.join(ROOT, "profiles", "sqnet_rate.txt"), "w").write(text)
