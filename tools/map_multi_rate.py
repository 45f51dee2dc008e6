#!/usr/bin/env python3
"""Rate of mapping one read to many candidates (scrappie_hip_map_multi_batch; a DESIGN.md record, not bench.py's `value`), and the
measurement the default pack size is chosen by.  10 000 synthetic reads of 4000 samples (synthetic rgrgr_r94 weights), Viterbi
scores, two shapes:
  A  24 candidates of 40 bases shared by every read (barcodes)
  B  8 candidates of about 400 bases per read: a sequence of the read's own and 7 edits of it (substitutions, deletions, insertions)
and three routes:
  (i)   Engine.map_to_sequence with every read repeated once per candidate -- the only way before this call existed
  (ii)  map_pack_cells = 0: the network once per read, k_map per candidate, one workgroup each
  (iii) packed: k_map_pack at pack_cells 256, 512, 1024, 2048 and the most a pack holds
Every route must give the same bits.  Best wall of `repeats` after a warm-up call, with scrappie_hip_map_timing's split of that call; routes are compared by the sum of
the split's three terms, the engine's own time for the call.
The rule: the default is the fastest of (iii) on shape A that is not slower than (ii) on shape B by more than 3 % (the box-to-box
spread, README); if no packed setting beats (ii) on shape A by more than that spread, packing does not pay.
usage: map_multi_rate.py [reads=10000] [samples=4000] [repeats=3] [out=profiles/map_multi_rate.txt]"""
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
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "map_multi_rate.txt")
SPREAD = 0.03
rng = np.random.default_rng(1)
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
sigs = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal


def bases(k):
    return "".join(rng.choice(list("ACGT"), k))


def edit(s):
    """a few substitutions, a deletion and an insertion"""
    b = list(s)
    for _ in range(3):
        b[int(rng.integers(len(b)))] = "ACGT"[int(rng.integers(4))]
    if rng.random() < 0.5:
        del b[int(rng.integers(len(b)))]
    if rng.random() < 0.5:
        b.insert(int(rng.integers(len(b))), "ACGT"[int(rng.integers(4))])
    return "".join(b)


shape_a = [bases(40) for _ in range(24)]
shape_b = []
for _ in range(n):
    own = bases(400)
    shape_b.append([own] + [edit(own) for _ in range(7)])
shapes = {"A": ([shape_a] * n, shape_a, "24 shared candidates of 40 bases"),
          "B": (shape_b, shape_b, "8 candidates of ~400 bases per read")}

eng = sa.Engine(0)
eng.load_model("rgrgr_r94", model.synthetic_model("rgrgr_r94", seed=1))
nblock = eng.read_blocks("rgrgr_r94", ns)
maxc = sa.map_pack_max_cells()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    fn()                                    # warm-up: arena, kernels, buffers at this shape
    best, split, res = None, None, None
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        w = time.perf_counter() - t0
        walls.append(w)
        if best is None or w < best:
            best, split, res = w, eng.map_timing(), r
    return best, walls, split, res


say("map_multi_rate: %d reads x %d samples (%d blocks), Viterbi scores, best wall of %d after a warm-up call; a pack holds at most %d cells"
    % (n, ns, nblock, reps, maxc))
device_ms = {}
for name, (lists, arg, what) in shapes.items():
    K = sum(len(c) for c in lists) / float(n)
    cells = float(nblock) * (n * sum(len(q) - 4 for q in lists[0]) if name == "A" else sum(len(q) - 4 for c in lists for q in c))
    say("shape %s: %s (%.0f candidates per read, %.3e DP cells)" % (name, what, K, cells))
    flat_s = [x for x, c in zip(sigs, lists) for _ in c]
    flat_q = [q for c in lists for q in c]
    w, walls, sp, res = timed(lambda: eng.map_to_sequence(flat_s, flat_q, viterbi=True, path=False))
    want = np.array([s for s, _ in res], dtype=np.float32)
    assert np.all(np.isfinite(want))
    say("  (i)   every read repeated per candidate: wall %.3f s (%s); network + S1 %.1f ms, k_map %.1f ms, results %.1f ms"
        % (w, ", ".join("%.3f" % x for x in walls), sp["network_ms"], sp["map_ms"], sp["walk_ms"]))
    del flat_s, flat_q, res
    for pc in (0, 256, 512, 1024, 2048, maxc):
        eng.debug_option("map_pack_cells", pc)
        w, walls, sp, res = timed(lambda: eng.map_to_sequences(sigs, arg, viterbi=True, path=False))
        got = np.concatenate([sc for sc, _, _ in res])
        assert got.tobytes() == want.tobytes(), (name, pc)
        device_ms[(name, pc)] = sp["network_ms"] + sp["map_ms"] + sp["walk_ms"]
        say("  %s wall %.3f s (%s); network + S1 %.1f ms, %s %.1f ms (%.3e cells/s), results %.1f ms"
            % ("(ii)  k_map per candidate:              " if pc == 0 else "(iii) packed, pack_cells %4d:           " % pc, w,
               ", ".join("%.3f" % x for x in walls), sp["network_ms"], "k_map" if pc == 0 else "k_map_pack", sp["map_ms"],
               cells / (sp["map_ms"] * 1e-3), sp["walk_ms"]))
    eng.debug_option("map_pack_cells", -1)
    w, walls, sp, res = timed(lambda: eng.map_to_sequences(sigs, arg, viterbi=True, path=True))
    say("  the default with the best candidate's path: wall %.3f s; network + S1 %.1f ms, k_map_pack + k_map %.1f ms, walk + results %.1f ms"
        % (w, sp["network_ms"], sp["map_ms"], sp["walk_ms"]))

packed = [pc for pc in (256, 512, 1024, 2048, maxc)]
ok = [pc for pc in packed if device_ms[("B", pc)] <= device_ms[("B", 0)] * (1 + SPREAD)]
say("by the engine's time for the call (the three terms summed; the wall adds Python's encoding of the sequences, the same for every route): packed settings not slower than (ii) on shape B by more than 3 %%: %s" % (ok or "none"))
if ok:
    pick = min(ok, key=lambda pc: device_ms[("A", pc)])
    gain = device_ms[("A", 0)] / device_ms[("A", pick)]
    say("fastest of them on shape A: pack_cells %d, %.1f ms against %.1f ms for (ii): %.2fx -- %s"
        % (pick, device_ms[("A", pick)], device_ms[("A", 0)], gain, "packing pays" if gain > 1 + SPREAD else "NOT beyond the spread: packing does not pay"))
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
