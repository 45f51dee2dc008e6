#!/usr/bin/env python3
"""Rate of the CRF mapping on the engine (scrappie_hip_map_batch with a flip-flop model; a DESIGN.md record, not bench.py's
`value`).  10 000 synthetic reads of 4000 samples (synthetic rnnrf_r94 weights), each mapped in Viterbi with its path to the
engine's own call of it -- the sequence decode_crf finds, so the score is decode_crf's -- unbanded and inside a diagonal band.
Reports the three times of scrappie_hip_map_timing, reads/s and DP cells/s (a cell: one B and one S value of one entry), and
writes them to the output file beside k_map's record for the transducer model (profiles/map_rate.txt).
usage: map_crf_rate.py [reads=10000] [samples=4000] [halfwidth=32] [repeats=3] [out=profiles/map_crf_rate.txt]"""
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
hw = int(sys.argv[3]) if len(sys.argv) > 3 else 32
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "map_crf_rate.txt")
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
sigs = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal
eng = sa.Engine(0)
eng.load_model("rnnrf_r94", model.synthetic_model("rnnrf_r94", seed=11))
nblock = eng.read_blocks("rnnrf_r94", ns)
calls = eng.basecall(sigs, "rnnrf_r94")
seqs = [c["bases"] if c and c["bases"] else "A" for c in calls]               # (a call of no base at all: one base, counted below)
empty = sum(1 for c in calls if not (c and c["bases"]))
lens = np.array([len(s) for s in seqs])
band = [sa.map_crf_diagonal_band(nblock, len(s), hw) for s in seqs]
width = float(np.mean([np.mean(hi.astype(np.int64) - lo.astype(np.int64)) for lo, hi in band[:64]]))

lines = ["map_crf_rate: %d reads x %d samples (%d blocks, %d entries), each mapped to its own call (%d to %d bases, mean %.1f; %d calls of no base mapped to 'A'), Viterbi + path"
         % (n, ns, nblock, nblock + 1, lens.min(), lens.max(), lens.mean(), empty)]
eng.map_to_sequence(sigs[:256], seqs[:256], model="rnnrf_r94", path=True)          # warm-up: arena, kernels
for name, bands, cells in (("unbanded", None, float(np.sum((lens + 1) * nblock))),
                           ("diagonal band, half-width %d (mean width %.1f cells)" % (hw, width), band, float(n) * nblock * min(width, lens.mean() + 1))):
    walls, splits = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = eng.map_to_sequence(sigs, seqs, model="rnnrf_r94", viterbi=True, path=True, bands=bands)
        walls.append(time.perf_counter() - t0)
        splits.append(eng.map_timing())
    assert all(np.isfinite(s) and p is not None and len(p) == nblock + 1 for s, p in res)
    if bands is None:       # decode_crf's score, bit for bit, unless the call lacks a base at the path's very last entry (crfpath_to_basecall reads nblock entries)
        same = sum(1 for (s, _), c in zip(res, calls) if c and c["bases"] and np.float32(s) == np.float32(c["score"]))
        assert all(not (c and c["bases"]) or np.float32(s) <= np.float32(c["score"]) for (s, _), c in zip(res, calls)), "above decode_crf's score"
        lines.append("unbanded: %d of %d scores are decode_crf's own in bits (the others' calls lack the base of the path's last entry)" % (same, n - empty))
    wall = min(walls)
    sp = splits[int(np.argmin(walls))]
    lines.append("%s: wall %.3f s (best of %d: %s) = %.0f reads/s, %.3e DP cells/s" % (name, wall, reps, ", ".join("%.3f" % w for w in walls), n / wall, cells / wall))
    lines.append("  per call: network + k_crf %.1f ms, k_map_crf %.1f ms, k_map_crf_walk + results %.1f ms (host clock, stream drained between stages)"
                 % (sp["network_ms"], sp["map_ms"], sp["walk_ms"]))
    lines.append("  k_map_crf alone: %.3e DP cells/s, %.0f reads/s" % (cells / (sp["map_ms"] * 1e-3), n / (sp["map_ms"] * 1e-3)))
lines.append("beside it, k_map on the transducer model (profiles/map_rate.txt): 10000 reads x 800 blocks x 396 states, k_map 28.6 ms = 1.107e+11 DP cells/s, 55775 reads/s end to end")
eng.close()
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
