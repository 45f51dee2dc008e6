#!/usr/bin/env python3
"""Rate of the sequence-local transducer mapping on the engine (scrappie_hip_map_post_local_batch; a DESIGN.md record, not
bench.py's `value`).  Synthetic rgrgr_r94 reads (synthetic weights) mapped INTO a random reference:
  (a) 10 000 reads of 4000 samples against one shared sequence of 100 kb,
  (b) 16 such reads against one of 5 Mb,
  (c) 64 reads of 40 000 samples against the 100 kb sequence: their windows cannot live in LDS, so the scratch home has a number,
(a) and (b) at several strides of the window cut -- LDS-resident ones, the largest among them, strides whose windows live in
device scratch, and one window per sequence on a small subset -- Viterbi scores alone and Viterbi with paths.  Reports the wall
time, the three times of scrappie_hip_map_timing, reads/s and DP cells/s: a cell is one position of one block of the SEQUENCE,
len x blocks per read, whatever the cut recomputes where windows overlap.  Every run after a warm-up call, the best of `repeats`.
usage: map_local_rate.py [reads_a=10000] [len_a=100000] [reads_b=16] [len_b=5000000] [samples=4000] [repeats=2] [reads_c=64] [samples_c=40000] [out=profiles/map_local_rate.txt]"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scrappie_amd as sa
from scrappie_amd import model, synth

arg = lambda k, d: type(d)(sys.argv[k]) if len(sys.argv) > k else d
na, la, nb, lb, ns, reps, nc, nsc = arg(1, 10000), arg(2, 100000), arg(3, 16), arg(4, 5000000), arg(5, 4000), arg(6, 2), arg(7, 64), arg(8, 40000)
out_path = arg(9, os.path.join(ROOT, "profiles", "map_local_rate.txt"))
MODEL, NR, K = "rgrgr_r94", 1025, 5
long_sig = synth.medmad_normalise(synth.synthetic_signal(max(ns, nsc) + 64 * 7, 5))
eng = sa.Engine(0)
eng.load_model(MODEL, model.synthetic_model(MODEL, seed=1))
nblock = eng.read_blocks(MODEL, ns)
reach = 2 * (nblock - 1)
M = sa.map_local_max_cells(NR)
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def run(sigs, ref, stride, path, reps=reps):
    eng.debug_option("map_local_stride", stride)
    walls, splits = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = eng.map_to_reference_transducer(sigs, ref, model=MODEL, viterbi=True, path=path)
        walls.append(time.perf_counter() - t0)
        splits.append(eng.map_timing())
    assert all(np.isfinite(r[0]) and (r[3] is not None) == path for r in res)
    k = int(np.argmin(walls))
    return walls[k], splits[k], walls, res


def split(sp, cells):
    return ("      network + S1 %.1f ms, plan + first pass %.1f ms (%.3e DP cells/s), second pass + walk + results %.1f ms"
            % (sp["network_ms"], sp["map_ms"], cells / (sp["map_ms"] * 1e-3), sp["walk_ms"]))


def sigs_of(n, nsamp):
    return [long_sig[(i % 64) * 7:(i % 64) * 7 + nsamp].copy() for i in range(n)]      # every read a different window of one signal


say("map_local_rate: %s reads of %d samples (%d blocks, a path reaches %d positions); with %d states an LDS window holds at most %d cells, so the largest LDS-resident stride is %d; the default stride is %d"
    % (MODEL, ns, nblock, reach, NR, M, M - reach, int(sa.lib().scrappie_hip_map_local_stride(la - K + 1, nblock, NR, -1))))
rng = np.random.default_rng(17)
refs = {}
first = {}
for shape, n, Lb in (("a", na, la), ("b", nb, lb)):
    sigs = sigs_of(n, ns)
    ref = refs.setdefault(Lb, "".join(np.array(list("ACGT"))[rng.integers(0, 4, Lb)]))
    L = Lb - K + 1
    default = int(sa.lib().scrappie_hip_map_local_stride(L, nblock, NR, -1))
    cells = float(n) * L * nblock
    say("shape (%s): %d reads against one shared sequence of %d bases (%d states): %.3e DP cells per pass" % (shape, n, Lb, L, cells))
    eng.map_to_reference_transducer(sigs[:min(n, 64)], ref[:20000], model=MODEL, viterbi=True, path=True)      # warm-up: arena, kernels
    base = None
    best = {}
    for stride in sorted({default, M - reach, 1800, 1600, 1200, 800, 400, 2 * nblock, 4 * nblock}, reverse=True):
        nwin = (L + stride - 1) // stride
        home = "scratch" if stride + reach > M else "LDS"
        for path in (False, True):
            wall, sp, walls, res = run(sigs, ref, stride, path)
            if base is None:
                base = [r[0] for r in res]
            assert [r[0] for r in res] == base, "the Viterbi score depends on the stride"
            say("  stride %5d%s%s (%d windows of <= %d cells per read, %s), Viterbi %s: wall %.3f s (best of %d: %s) = %.1f reads/s, %.3e DP cells/s"
                % (stride, " (the default)" if stride == default else "", " (the largest in LDS)" if stride == M - reach else "", nwin, min(stride + reach, L), home,
                   "with paths" if path else "scores", wall, reps, ", ".join("%.3f" % w for w in walls), n / wall, cells / wall))
            say(split(sp, cells))
            if not path:
                best[stride] = sp["map_ms"]
    first[shape] = best
    m = min(n, 64 if L <= 200000 else 16)                                               # one window per sequence, rows in device scratch
    for path in (False, True):
        wall, sp, walls, res = run(sigs[:m], ref, 0, path, reps=1)
        assert [r[0] for r in res] == base[:m], "the Viterbi score depends on the stride"
        c1 = float(m) * L * nblock
        say("  one window of %d cells per read in scratch, %d reads, Viterbi %s: wall %.3f s (one run) = %.1f reads/s, %.3e DP cells/s"
            % (L, m, "with paths" if path else "scores", wall, m / wall, c1 / wall))
        say(split(sp, c1))
    eng.debug_option("map_local_stride", -1)
# (c): long reads, whose windows cannot live in LDS
sigs = sigs_of(nc, nsc)
nbc = eng.read_blocks(MODEL, nsc)
ref = refs[la]
L = la - K + 1
dc = int(sa.lib().scrappie_hip_map_local_stride(L, nbc, NR, -1))
cells = float(nc) * L * nbc
say("shape (c): %d reads of %d samples (%d blocks) against the sequence of %d bases: %.3e DP cells per pass; default stride %d, windows of <= %d cells in scratch"
    % (nc, nsc, nbc, la, cells, dc, min(dc + 2 * (nbc - 1), L)))
for path in (False, True):
    wall, sp, walls, res = run(sigs, ref, -1, path)
    say("  Viterbi %s: wall %.3f s (best of %d: %s) = %.1f reads/s, %.3e DP cells/s" % ("with paths" if path else "scores", wall, reps, ", ".join("%.3f" % w for w in walls), nc / wall, cells / wall))
    say(split(sp, cells))
# the rule for the default: the fastest first pass on (a), provided it is within 3 % of the fastest on (b)
fa = min(first["a"], key=first["a"].get)
fb = min(first["b"], key=first["b"].get)
say("fastest first pass (scores): (a) stride %d (%.1f ms), (b) stride %d (%.1f ms); (a)'s fastest on (b): %.1f ms = %.1f %% above (b)'s fastest"
    % (fa, first["a"][fa], fb, first["b"][fb], first["b"][fa], 100.0 * (first["b"][fa] / first["b"][fb] - 1.0)))
eng.close()
