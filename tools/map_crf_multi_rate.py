#!/usr/bin/env python3
"""Rate of mapping one flip-flop (CRF) read to many candidates (scrappie_hip_map_crf_multi_batch; a DESIGN.md record, not bench.py's
`value`), and the measurement the default pack size is chosen by.  10 000 synthetic reads (synthetic rnnrf_r94 weights), Viterbi
scores, two shapes:
  A  16 candidates of about 150 bases shared by every read, reads of 1000 samples (200 blocks): a short amplicon panel
  B  8 candidates per read, reads of 4000 samples: the read's own call and 7 edits of it (substitutions, deletions, insertions)
and three routes:
  (i)   Engine.map_to_sequence(model="rnnrf_r94") with every read repeated once per candidate -- the only way before this call existed
  (ii)  map_crf_pack_cells = 0: the network once per read, k_map_crf per candidate, one workgroup each
  (iii) packed: k_map_crf_pack at pack_cells 256, 512, 1024, 2048 and the most a pack holds
Every route must give the same bits.  Best wall of `repeats` after a warm-up call, with scrappie_hip_map_timing's split of that call;
routes are compared by the sum of the split's three terms, the engine's own time for the call.
The rule (tools/map_multi_rate.py states it): the default is the fastest of (iii) on shape A that is not slower than (ii) on shape B by
more than 3 % (the box-to-box spread, README); if none qualifies, or none beats (ii) on shape A by more than that spread, packing does
not pay and the default is route (ii).
usage: map_crf_multi_rate.py [reads=10000] [samples=4000] [repeats=3] [out=profiles/map_crf_multi_rate.txt]"""
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
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "map_crf_multi_rate.txt")
SPREAD = 0.03
MODEL = "rnnrf_r94"
rng = np.random.default_rng(1)
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
sigs_b = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal
sigs_a = [x[:min(ns, 1000)] for x in sigs_b]


def bases(k):
    return "".join(rng.choice(list("ACGT"), k))


def edit(s):
    """a few substitutions, a deletion and an insertion"""
    b = list(s)
    for _ in range(3):
        b[int(rng.integers(len(b)))] = "ACGT"[int(rng.integers(4))]
    if rng.random() < 0.5 and len(b) > 1:
        del b[int(rng.integers(len(b)))]
    if rng.random() < 0.5:
        b.insert(int(rng.integers(len(b))), "ACGT"[int(rng.integers(4))])
    return "".join(b)


eng = sa.Engine(0)
eng.load_model(MODEL, model.synthetic_model(MODEL, seed=11))
nb_a, nb_b = eng.read_blocks(MODEL, len(sigs_a[0])), eng.read_blocks(MODEL, ns)
shape_a = [bases(min(int(rng.integers(140, 161)), nb_a + 1)) for _ in range(16)]
calls = {}
for i in range(min(n, 64)):                  # the reads are 64 windows of one signal: 64 calls
    c = eng.basecall([sigs_b[i]], MODEL)[0]
    calls[i] = c["bases"] if c is not None and len(c["bases"]) >= 8 else bases(max(8, nb_b // 3))
shape_b = []
for i in range(n):
    own = calls[i % 64]
    shape_b.append([own] + [edit(own) for _ in range(7)])
shapes = {"A": (sigs_a, [shape_a] * n, shape_a, nb_a, "16 shared candidates of about 150 bases, reads of %d samples" % len(sigs_a[0])),
          "B": (sigs_b, shape_b, shape_b, nb_b, "the read's own call and 7 edits of it, reads of %d samples" % ns)}
maxc = sa.map_crf_pack_max_cells()
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


say("map_crf_multi_rate: %d reads, Viterbi scores, best wall of %d after a warm-up call; a pack holds at most %d cells" % (n, reps, maxc))
device_ms = {}
for name, (sigs, lists, arg, nblock, what) in shapes.items():
    K = sum(len(c) for c in lists) / float(n)
    cells = float(nblock) * (n * sum(len(q) + 1 for q in lists[0]) if name == "A" else sum(len(q) + 1 for c in lists for q in c))
    say("shape %s: %s (%d blocks, %.0f candidates per read of %.0f bases on average, %.3e DP cells)"
        % (name, what, nblock, K, sum(len(q) for q in lists[0]) / float(len(lists[0])), cells))
    flat_s = [x for x, c in zip(sigs, lists) for _ in c]
    flat_q = [q for c in lists for q in c]
    w, walls, sp, res = timed(lambda: eng.map_to_sequence(flat_s, flat_q, model=MODEL, viterbi=True, path=False))
    want = np.array([s for s, _ in res], dtype=np.float32)
    assert np.all(np.isfinite(want))
    device_ms[(name, "i")] = sp["network_ms"] + sp["map_ms"] + sp["walk_ms"]
    say("  (i)   every read repeated per candidate: wall %.3f s (%s); network + k_crf %.1f ms, k_map_crf %.1f ms, results %.1f ms"
        % (w, ", ".join("%.3f" % x for x in walls), sp["network_ms"], sp["map_ms"], sp["walk_ms"]))
    del flat_s, flat_q, res
    for pc in (0, 256, 512, 1024, 2048, maxc):
        eng.debug_option("map_crf_pack_cells", pc)
        w, walls, sp, res = timed(lambda: eng.map_to_sequences_crf(sigs, arg, model=MODEL, viterbi=True, path=False))
        got = np.concatenate([sc for sc, _, _ in res])
        assert got.tobytes() == want.tobytes(), (name, pc)
        device_ms[(name, pc)] = sp["network_ms"] + sp["map_ms"] + sp["walk_ms"]
        say("  %s wall %.3f s (%s); network + k_crf %.1f ms, %s %.1f ms (%.3e cells/s), results %.1f ms"
            % ("(ii)  k_map_crf per candidate:          " if pc == 0 else "(iii) packed, pack_cells %4d:           " % pc, w,
               ", ".join("%.3f" % x for x in walls), sp["network_ms"], "k_map_crf" if pc == 0 else "k_map_crf_pack", sp["map_ms"],
               cells / (sp["map_ms"] * 1e-3), sp["walk_ms"]))
    eng.debug_option("map_crf_pack_cells", -1)
    w, walls, sp, res = timed(lambda: eng.map_to_sequences_crf(sigs, arg, model=MODEL, viterbi=True, path=True))
    say("  the built-in default with the best candidate's path: wall %.3f s; network + k_crf %.1f ms, k_map_crf_pack + k_map_crf %.1f ms, walk + results %.1f ms"
        % (w, sp["network_ms"], sp["map_ms"], sp["walk_ms"]))

packed = [pc for pc in (256, 512, 1024, 2048, maxc)]
ok = [pc for pc in packed if device_ms[("B", pc)] <= device_ms[("B", 0)] * (1 + SPREAD)]
say("by the engine's time for the call (the three terms summed; the wall adds Python's encoding of the sequences, the same for every route): packed settings not slower than (ii) on shape B by more than 3 %%: %s" % (ok or "none"))
if ok:
    pick = min(ok, key=lambda pc: device_ms[("A", pc)])
    gain = device_ms[("A", 0)] / device_ms[("A", pick)]
    say("fastest of them on shape A: pack_cells %d, %.1f ms against %.1f ms for (ii): %.2fx -- %s"
        % (pick, device_ms[("A", pick)], device_ms[("A", 0)], gain, "packing pays" if gain > 1 + SPREAD else "NOT beyond the spread: packing does not pay, the default is route (ii)"))
    say("against (i), repeating the read per candidate: %.1fx on shape A (%.1f ms), %.1fx on shape B (%.1f ms against %.1f ms)"
        % (device_ms[("A", "i")] / device_ms[("A", pick)], device_ms[("A", "i")], device_ms[("B", "i")] / device_ms[("B", pick)], device_ms[("B", "i")], device_ms[("B", pick)]))
else:
    say("none qualifies: the default is route (ii), map_crf_pack_cells = 0")
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
