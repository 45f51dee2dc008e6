#!/usr/bin/env python3
"""Rate of searching short sequences inside flip-flop reads (scrappie_hip_find_batch, k_crf_find; a DESIGN.md record, not bench.py's
`value`), and the measurement the default pack size is chosen by.  10 000 synthetic reads of 4000 samples (synthetic rnnrf_r94
weights), two shapes:
  a  24 shared motifs of 40 bases (barcodes), with and without positions
  b  96 shared motifs of 24 bases (primers), with positions
each at crf_find_cells 128, 256, 512, 1024 and the most a pack holds, with scrappie_hip_map_timing's split of the best call; every
setting must give the same bits.  Beside them the same reads through Engine.basecall (this change does not touch the basecaller):
what the search adds to a call.
The rule: the default is the fastest setting on (a) with positions that is not slower on (b) than (b)'s best by more than 3 % (the
box-to-box spread, README), by the engine's own time for the call (the split's three terms summed).
usage: crf_find_rate.py [reads=10000] [samples=4000] [repeats=3] [out=profiles/crf_find_rate.txt]"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scrappie_amd as sa
from scrappie_amd import model, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "crf_find_rate.txt")
SPREAD = 0.03
rng = np.random.default_rng(1)
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
sigs = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal


def bases(k):
    return "".join(rng.choice(list("ACGT"), k))


shapes = {"a": ([bases(40) for _ in range(24)], "24 shared motifs of 40 bases"),
          "b": ([bases(24) for _ in range(96)], "96 shared motifs of 24 bases")}

eng = sa.Engine(0)
eng.load_model("rnnrf_r94", model.synthetic_model("rnnrf_r94", seed=11))
nblock = eng.read_blocks("rnnrf_r94", ns)
maxc = sa.crf_find_max_cells()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, split=True):
    fn()                                    # warm-up: arena, kernels, buffers at this shape
    best, sp, res, walls = None, None, None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        w = time.perf_counter() - t0
        walls.append(w)
        if best is None or w < best:
            best, sp, res = w, (eng.map_timing() if split else None), r
    return best, walls, sp, res


say("crf_find_rate: %d reads x %d samples (%d blocks), best wall of %d after a warm-up call; a pack holds at most %d cells"
    % (n, ns, nblock, reps, maxc))
w, walls, _, calls = timed(lambda: eng.basecall(sigs, "rnnrf_r94"), split=False)
say("Engine.basecall on the same reads: wall %.3f s (%s)" % (w, ", ".join("%.3f" % x for x in walls)))
del calls
device_ms = {}
settings = (128, 256, 512, 1024, maxc)
for name, pos in (("a", True), ("a", False), ("b", True)):
    motifs, what = shapes[name]
    cells = float(n) * nblock * (5 + sum(len(m) + 4 for m in motifs))
    say("shape %s, %s: %s (%.3e cells x blocks, the read's own five once per read)" % (name, "with positions" if pos else "scores only", what, cells))
    want = None
    for pc in settings:
        eng.debug_option("crf_find_cells", pc)
        npack = sa.crf_find_plan([len(m) for m in motifs], pc)[0]
        w, walls, sp, res = timed(lambda: eng.find_sequences(sigs, motifs, positions=pos))
        got = np.concatenate([r[0] for r in res]).tobytes()
        if want is None:
            want = got
        assert got == want, (name, pos, pc)
        device_ms[(name, pos, pc)] = sp["network_ms"] + sp["map_ms"] + sp["walk_ms"]
        say("  crf_find_cells %4d (%2d packs per read): wall %.3f s (%s); network + k_crf %.1f ms, k_crf_find %.1f ms (%.3e cells/s), results %.1f ms"
            % (pc, npack, w, ", ".join("%.3f" % x for x in walls), sp["network_ms"], sp["map_ms"], cells / (sp["map_ms"] * 1e-3), sp["walk_ms"]))
        del res
    eng.debug_option("crf_find_cells", -1)

best_b = min(device_ms[("b", True, pc)] for pc in settings)
ok = [pc for pc in settings if device_ms[("b", True, pc)] <= best_b * (1 + SPREAD)]
pick = min(ok, key=lambda pc: device_ms[("a", True, pc)])
say("by the engine's time for the call (the three terms summed): settings within 3 %% of (b)'s best (%.1f ms): %s; the fastest of them on (a) with positions: crf_find_cells %d (%.1f ms)"
    % (best_b, ok, pick, device_ms[("a", True, pick)]))
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
