#!/usr/bin/env python3
"""Rate of scoring every single-base edit of a read's own call INSIDE A BAND (scrappie_hip_map_crf_edits_banded_batch; a DESIGN.md
record, not bench.py's `value`).  Shape B of tools/crf_edits_rate.py: 10 000 synthetic reads of 4000 samples (800 blocks, synthetic
rnnrf_r94 weights), each against its own call of about 712 bases, Viterbi and forward, in one process: unbanded
(scrappie_hip_map_crf_edits_batch), then in the bands of half-width 8, 32 and 128 around the reads' Viterbi paths
(Engine.map_to_sequence with path=True, map_crf_path_band), then in the diagonal band of half-width 32.  Best wall of `repeats` after a
warm-up call, with scrappie_hip_crf_edits_timing's split of that call: the three kernels by events on the stream, the row bytes the
launches kept -- each against the unbanded figure of the same run -- and the band's share of the lattice's cells.  Then, on the first
read in its path band of half-width 32: the 20 edits it scores highest scored again, unbanded, by map_to_sequences_crf's engine.
usage: crf_edits_band_rate.py [reads=10000] [samples=4000] [repeats=2] [out=profiles/crf_edits_band_rate.txt]"""
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
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "crf_edits_band_rate.txt")
MODEL = "rnnrf_r94"
rng = np.random.default_rng(1)
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
sigs = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, split):
    fn()                                    # warm-up: arena, kernels, buffers at this shape
    best, sp, res, walls = None, None, None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        w = time.perf_counter() - t0
        walls.append(w)
        if best is None or w < best:
            best, sp, res = w, split(), r
    return best, walls, sp, res


eng = sa.Engine(0)
eng.load_model(MODEL, model.synthetic_model(MODEL, seed=11))
nblock = eng.read_blocks(MODEL, ns)
maxL = int(sa.lib().scrappie_hip_map_crf_lds_max_seq())
calls = {}
for i in range(min(n, 64)):                  # the reads are 64 windows of one signal: 64 calls
    c = eng.basecall([sigs[i]], MODEL)[0]
    b = c["bases"] if c is not None and len(c["bases"]) >= 8 else "".join(rng.choice(list("ACGT"), max(8, nblock // 3)))
    calls[i] = sa.encode_bases(b[:maxL], 1).astype(np.int32)
nu = min(n, 64)
seqs = [calls[i % 64] for i in range(n)]
nedit = sum(9 * len(s) + 4 for s in seqs)
full_bytes = sum(int(sa.lib().scrappie_hip_crf_edits_row_bytes(len(s), nblock)) for s in seqs)
full_cells = sum((nblock + 1) * (len(s) + 1) for s in seqs)
# the Viterbi paths of the 64 different reads, once: the bands are built around them
mapped = eng.map_to_sequence(sigs[:nu], ["".join("ACGT"[b] for b in calls[i]) for i in range(nu)], model=MODEL, viterbi=True, path=True)
paths = [p for _, p in mapped]
assert all(p is not None for p in paths)
configs = [("unbanded", None)]
for h in (8, 32, 128):
    configs.append(("path band, half-width %d" % h, [sa.map_crf_path_band(paths[i], len(calls[i]), h) for i in range(nu)]))
configs.append(("diagonal band, half-width 32", [sa.map_crf_diagonal_band(nblock, len(calls[i]), 32) for i in range(nu)]))
say("crf_edits_band_rate: %d reads of %d samples (%d blocks), each against its own call (%.0f bases on average): %.3e edits; best wall of %d after a warm-up call"
    % (n, ns, nblock, sum(len(s) for s in seqs) / float(n), nedit, reps))
ref = {}
first = None
for name, b64 in configs:
    bands = None if b64 is None else [b64[i % 64] for i in range(n)]
    if bands is None:
        row_bytes, share = full_bytes, 1.0
    else:
        row_bytes = sum(sa.crf_edits_band_row_bytes(*b64[i % 64]) for i in range(n))
        share = sum(int(np.sum(b64[i % 64][1].astype(np.int64) - b64[i % 64][0].astype(np.int64))) for i in range(n)) / float(full_cells)
    say("%s: %.1f %% of the lattice's cells, %.2f GB of rows (%.1f %% of the unbanded %.2f GB)" % (name, 100 * share, row_bytes / 1e9, 100.0 * row_bytes / full_bytes, full_bytes / 1e9))
    for vit in (True, False):
        w, walls, k, res = timed(lambda: eng.score_edits(sigs, seqs, model=MODEL, viterbi=vit, bands=bands), eng.crf_edits_timing)
        ks = k["rows_forward_ms"] + k["rows_backward_ms"] + k["edits_ms"]
        assert k["row_bytes"] == row_bytes, (k["row_bytes"], row_bytes)
        finite = sum(1 for r in res[:64] if np.isfinite(r[0]))
        if bands is None:
            ref[vit] = (k["rows_forward_ms"], k["rows_backward_ms"], k["edits_ms"], ks)
        u = ref[vit]
        say("  %s wall %.3f s (%s); k_crf_edits_rows forward %.1f ms, backward %.1f ms, k_crf_edits %.1f ms: %.1f ms in the kernels, %.3e edits/s; %d launch(es); base finite on %d of the first 64 reads"
            % ("viterbi:" if vit else "forward:", w, ", ".join("%.3f" % x for x in walls), k["rows_forward_ms"], k["rows_backward_ms"], k["edits_ms"], ks,
               nedit / (ks * 1e-3), k["launches"], finite))
        if bands is not None:
            say("           against unbanded: forward rows x%.3f, backward rows x%.3f, k_crf_edits x%.3f, the three x%.3f"
                % (k["rows_forward_ms"] / u[0], k["rows_backward_ms"] / u[1], k["edits_ms"] / u[2], ks / u[3]))
        if vit and name.endswith("half-width 32") and name.startswith("path"):
            first = res[0]

# read 0 in its path band of half-width 32: the 20 highest edits again, unbanded and exact
edits = [("sub", i, c) for i in range(len(seqs[0])) for c in range(4)] + [("del", i, None) for i in range(len(seqs[0]))] + \
        [("ins", i, c) for i in range(len(seqs[0]) + 1) for c in range(4)]
flat = np.concatenate([np.ravel(first[1]), np.ravel(first[2]), np.ravel(first[3])])
top = [int(j) for j in np.argsort(-np.where(np.isnan(flat), -np.inf, flat), kind="stable")[:20]]
((again, _, _),) = eng.map_to_sequences_crf([sigs[0]], [[sa.apply_edit(seqs[0], *edits[j]) for j in top]], model=MODEL, viterbi=True, path=False)
again = np.asarray(again, dtype=np.float64)
diff = np.abs(flat[top].astype(np.float64) - again)
say("read 0 in its path band of half-width 32, its 20 highest edits scored again by map_to_sequences_crf (unbanded): largest |difference| %.3g on scores near %.1f (%.2g relative)"
    % (float(diff.max()), float(first[0]), float(diff.max()) / abs(float(first[0]))))
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
