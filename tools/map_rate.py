#!/usr/bin/env python3
"""Rate of block-based mapping on the engine (scrappie_hip_map_batch; a DESIGN.md record, not bench.py's `value`).
10 000 synthetic reads of 4000 samples (synthetic rgrgr_r94 weights), each mapped in Viterbi with its path to a
~400-base sequence of its own (random bases, seeded; the weights are random, so what is measured is the work, not the
biology).  Reports reads/s, DP cells/s, the split of launch-group time between network + S1 and the map kernels, and
the HBM bytes the map kernel moves (counted from the layout: the posterior pieces each tile touches, the traceback).
usage: map_rate.py [reads=10000] [samples=4000] [bases=400] [repeats=3]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scrappie_amd as sa
from scrappie_amd import model, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
nbase = int(sys.argv[3]) if len(sys.argv) > 3 else 400
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
rng = np.random.default_rng(1)
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
sigs = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal
seqs = ["".join(rng.choice(list("ACGT"), nbase)) for _ in range(n)]
eng = sa.Engine(0)
eng.load_model("rgrgr_r94", model.synthetic_model("rgrgr_r94", seed=1))
nblock = eng.read_blocks("rgrgr_r94", ns)
L = nbase - 5 + 1

eng.map_to_sequence(sigs[:256], seqs[:256], path=True)          # warm-up: arena, kernels
walls, splits = [], []
for _ in range(reps):
    t0 = time.perf_counter()
    res = eng.map_to_sequence(sigs, seqs, viterbi=True, path=True)
    walls.append(time.perf_counter() - t0)
    splits.append(eng.map_timing())
assert all(np.isfinite(s) and p is not None and len(p) == nblock for s, p in res)
wall = min(walls)
sp = splits[int(np.argmin(walls))]
cells = float(n) * nblock * L

# HBM bytes of k_map, from the layout (sh_map.h): per column block a tile of 16 reads touches, in each 1 KiB chunk, the
# 256-byte quarter (16 lanes x 16 bytes) of every group of 4 states one of its reads maps to (+ stay), and the row sums;
# each read writes W = 4 ceil(L / 64) traceback words per block (+ END bits) and reads its codes once.
codes = [sa.encode_bases(s, 5) for s in seqs]
pieces = 0
for t in range(0, n, 16):
    u = set()
    for c in codes[t:t + 16]:
        u.update((c >> 2).tolist())
    u.add(1024 >> 2)
    pieces += len(u)
post_read = pieces * 256 * nblock + (n // 16) * nblock * 64
W = 4 * ((L + 63) // 64)
tb_write = n * (nblock * W + ((nblock + 31) // 32 + 3) // 4 * 4) * 4
map_bytes = post_read + tb_write + n * L * 4
post_written = (n // 16) * nblock * (65 * 1024 + 64)        # what S1 writes (4^5 + 1 states in 65 chunks) and nobody reads whole

print("map_rate: %d reads x %d samples (%d blocks), sequences of %d bases (%d states), Viterbi + path" % (n, ns, nblock, nbase, L))
print("wall %.3f s (best of %d: %s) = %.0f reads/s, %.3e DP cells/s" % (wall, reps, ", ".join("%.3f" % w for w in walls), n / wall, cells / wall))
print("per call: network + S1 %.1f ms, k_map %.1f ms, k_map_walk + results %.1f ms (host clock, stream drained between stages)"
      % (sp["network_ms"], sp["map_ms"], sp["walk_ms"]))
print("k_map alone: %.3e DP cells/s" % (cells / (sp["map_ms"] * 1e-3)))
print("k_map HBM bytes (layout count): posterior pieces %.2f GB + traceback %.2f GB + codes %.3f GB = %.2f GB -> %.2f TB/s over k_map's time"
      % (post_read / 1e9, tb_write / 1e9, n * L * 4 / 1e9, map_bytes / 1e9, map_bytes / (sp["map_ms"] * 1e-3) / 1e12))
print("posterior materialised by S1: %.2f GB written (the fused decoder never stores it)" % (post_written / 1e9))
eng.close()
