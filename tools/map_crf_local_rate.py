#!/usr/bin/env python3
"""Rate of the sequence-local CRF mapping on the engine (scrappie_hip_map_local_batch; a DESIGN.md record, not bench.py's
`value`).  Synthetic rnnrf_r94 reads of 4000 samples (synthetic weights) mapped INTO a random reference:
  (a) 10 000 reads against one shared sequence of 100 kb,
  (b) 16 reads against one of 5 Mb,
each at several strides of the window cut -- LDS-resident ones, the default and the largest among them, and one window per sequence with its rows in
device scratch (on fewer reads where its scratch rows and traceback would not fit) -- Viterbi scores alone and Viterbi with paths.
Reports the wall time, the three times of scrappie_hip_map_timing, reads/s and DP cells/s: a cell is one (B, S) pair of one entry
of the SEQUENCE, (len + 1) x blocks per read, whatever the cut recomputes where windows overlap.
usage: map_crf_local_rate.py [reads_a=10000] [len_a=100000] [reads_b=16] [len_b=5000000] [samples=4000] [repeats=2] [out=profiles/map_crf_local_rate.txt]"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scrappie_amd as sa
from scrappie_amd import model, synth

arg = lambda k, d: type(d)(sys.argv[k]) if len(sys.argv) > k else d
na, la, nb, lb, ns, reps = arg(1, 10000), arg(2, 100000), arg(3, 16), arg(4, 5000000), arg(5, 4000), arg(6, 2)
out_path = arg(7, os.path.join(ROOT, "profiles", "map_crf_local_rate.txt"))
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
eng = sa.Engine(0)
eng.load_model("rnnrf_r94", model.synthetic_model("rnnrf_r94", seed=11))
nblock = eng.read_blocks("rnnrf_r94", ns)
M = sa.map_crf_local_max_cells()
default = int(sa.lib().scrappie_hip_map_crf_local_stride(la, nblock, -1))
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def run(sigs, ref, stride, path, reps=reps):
    eng.debug_option("map_crf_local_stride", stride)
    walls, splits = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = eng.map_to_reference(sigs, ref, viterbi=True, path=path)
        walls.append(time.perf_counter() - t0)
        splits.append(eng.map_timing())
    assert all(np.isfinite(r[0]) and (r[3] is not None) == path for r in res)
    k = int(np.argmin(walls))
    return walls[k], splits[k], walls, res


say("map_crf_local_rate: rnnrf_r94 reads of %d samples (%d blocks, %d entries); an LDS window holds at most %d cells, the default stride is %d start cells (window %d cells)"
    % (ns, nblock, nblock + 1, M, default, default + nblock))
rng = np.random.default_rng(17)
for shape, n, L in (("a", na, la), ("b", nb, lb)):
    sigs = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal
    ref = "".join(np.array(list("ACGT"))[rng.integers(0, 4, L)])
    cells = float(n) * (L + 1) * nblock
    say("shape (%s): %d reads against one shared sequence of %d bases: %.3e DP cells per pass" % (shape, n, L, cells))
    eng.map_to_reference(sigs[:min(n, 64)], ref[:20000], viterbi=True, path=True)      # warm-up: arena, kernels
    base = None
    for stride in sorted({default, M - nblock, 1900, 1600, 1234, 800, 400}, reverse=True):
        nwin = (L + stride) // stride
        for path in (False, True):
            wall, sp, walls, res = run(sigs, ref, stride, path)
            if base is None:
                base = [r[0] for r in res]
            assert [r[0] for r in res] == base, "the Viterbi score depends on the stride"
            say("  stride %5d%s (%d windows of <= %d cells per read), Viterbi %s: wall %.3f s (best of %d: %s) = %.1f reads/s, %.3e DP cells/s"
                % (stride, " (the default)" if stride == default else " (the largest in LDS)" if stride == M - nblock else "", nwin, min(stride + nblock, L + 1), "with paths" if path else "scores", wall, reps, ", ".join("%.3f" % w for w in walls), n / wall, cells / wall))
            say("      network + k_crf %.1f ms, plan + first pass %.1f ms (%.3e DP cells/s), second pass + walk + results %.1f ms"
                % (sp["network_ms"], sp["map_ms"], cells / (sp["map_ms"] * 1e-3), sp["walk_ms"]))
    m = min(n, 64 if L <= 200000 else 16)                                               # one window per sequence, rows in device scratch
    for path in (False, True):
        wall, sp, walls, res = run(sigs[:m], ref, 0, path, reps=1)
        assert [r[0] for r in res] == base[:m], "the Viterbi score depends on the stride"
        c1 = float(m) * (L + 1) * nblock
        say("  one window of %d cells per read in scratch, %d reads, Viterbi %s: wall %.3f s (one run) = %.1f reads/s, %.3e DP cells/s"
            % (L + 1, m, "with paths" if path else "scores", wall, m / wall, c1 / wall))
        say("      network + k_crf %.1f ms, plan + first pass %.1f ms (%.3e DP cells/s), second pass + walk + results %.1f ms"
            % (sp["network_ms"], sp["map_ms"], c1 / (sp["map_ms"] * 1e-3), sp["walk_ms"]))
    eng.debug_option("map_crf_local_stride", -1)
say("beside it, the global k_map_crf (profiles/map_crf_rate.txt): 10000 reads x 800 blocks x 713 cells, k_map_crf 9.2 ms = 6.196e+11 DP cells/s")
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
