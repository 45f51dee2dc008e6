#!/usr/bin/env python3
"""Rate of scoring every single-base edit of a sequence for a transducer model INSIDE A BAND (scrappie_hip_map_edits_banded_batch; a
DESIGN.md record, not bench.py's `value`), on tools/map_edits_rate.py's shape and in one process: 10 000 synthetic reads of 4000
samples (800 blocks, synthetic rgrgr_r94 weights), each against its own call -- or, where the synthetic weights call it in fewer than
8 bases, a random sequence of a third of its blocks in bases.  The runs: unbanded; path bands of half-width 8, 32 and 128 states
around the reads' Viterbi paths (scrappie_hip_map_path_band on the paths of scrappie_hip_map_batch); scrappy's diagonal band of 32.
Each banded run at 64 and at 256 positions per workgroup of k_map_edits (the debug option "map_edits_band_width"), Viterbi and forward.
The columns: cells in the bands, row bytes, the three kernels by events on the stream (scrappie_hip_map_edits_timing; the best of
`repeats` calls after a warm-up call), edits/s; ratios are to the unbanded figures of the same run.  Then the 20 highest edits of read
0 in its path band of 32 scored again, unbanded, by map_post_to_sequences.
usage: map_edits_band_rate.py [reads=10000] [samples=4000] [repeats=2] [out=profiles/map_edits_band_rate.txt]"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scrappie_amd as sa
from scrappie_amd import model, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
ns = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "map_edits_band_rate.txt")
MODEL, K = "rgrgr_r94", 5
rng = np.random.default_rng(1)
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
sigs = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def text(codes):
    return "".join("ACGT"[b] for b in codes)


eng = sa.Engine(0)
eng.load_model(MODEL, model.synthetic_model(MODEL, seed=1))
nblock = eng.read_blocks(MODEL, ns)
maxL = int(sa.lib().scrappie_hip_map_edits_max_bases(K))
calls = {}
for i in range(min(n, 64)):                  # the reads are 64 windows of one signal: 64 calls
    c = eng.basecall([sigs[i]], MODEL)[0]
    b = c["bases"] if c is not None and len(c["bases"]) >= 8 else "".join(rng.choice(list("ACGT"), max(8, nblock // 3)))
    calls[i] = sa.encode_bases(b[:maxL], 1).astype(np.int32)
seqs = [calls[i % 64] for i in range(n)]
nedit = sum(9 * len(s) + 4 for s in seqs)
m = min(n, 64)
paths = [p for sc, p in eng.map_to_sequence(sigs[:m], [text(s) for s in seqs[:m]], model=MODEL, viterbi=True, path=True)]
assert all(p is not None for p in paths)


def bands_of(kind, h):
    if kind == "path":
        made = [sa.map_path_band(paths[i], len(seqs[i]) - K + 1, h) for i in range(m)]
    else:
        made = [sa.diagonal_bands(h, nblock, len(seqs[i]) - K + 1) for i in range(m)]
    return [made[i % m] for i in range(n)]


def run(vit, bands, width):
    """the best of `reps` calls by the three kernels' time: (timing, results)"""
    eng.debug_option("map_edits_band_width", width)
    try:
        fn = lambda: eng.score_edits_transducer(sigs, seqs, model=MODEL, viterbi=vit, bands=bands)
        fn()                                # warm-up: arena, kernels, buffers at this shape
        best, res = None, None
        for _ in range(reps):
            r = fn()
            k = eng.map_edits_timing()
            k["ms"] = k["rows_forward_ms"] + k["rows_backward_ms"] + k["edits_ms"]
            if best is None or k["ms"] < best["ms"]:
                best, res = k, r
        return best, res
    finally:
        eng.debug_option("map_edits_band_width", 0)


say("map_edits_band_rate: %d reads of %d samples (%d blocks), each against its sequence (%.0f bases on average): %.3e edits; the three kernels by events, best of %d after a warm-up call"
    % (n, ns, nblock, sum(len(s) for s in seqs) / float(n), nedit, reps))
say("  %-8s %-14s %5s %11s %9s %9s %9s %9s %9s %7s %11s" % ("form", "band", "width", "cells", "rows GB", "rows fwd", "rows bwd", "k_map_ed", "three ms", "ratio", "edits/s"))
full_cells = sum((len(s) - K + 1) * nblock for s in seqs)
keep = {}
for vit in (True, False):
    form = "viterbi" if vit else "forward"
    k0, res0 = run(vit, None, 0)
    assert all(np.isfinite(r[0]) for r in res0[:64])
    say("  %-8s %-14s %5s %11.3e %9.2f %9.1f %9.1f %9.1f %9.1f %7s %11.3e"
        % (form, "none", "256", full_cells, k0["row_bytes"] / 1e9, k0["rows_forward_ms"], k0["rows_backward_ms"], k0["edits_ms"], k0["ms"], "1.000", nedit / (k0["ms"] * 1e-3)))
    for kind, h in (("path", 8), ("path", 32), ("path", 128), ("diagonal", 32)):
        bands = bands_of(kind, h)
        cells = sum(int(np.sum(b[1].astype(np.int64) - b[0].astype(np.int64))) for b in bands)
        for width in (64, 256):
            k, res = run(vit, bands, width)
            assert all(np.isfinite(r[0]) and np.any(np.isfinite(r[1])) for r in res[:64]), (kind, h, width)      # (a band that is not valid for its read would be all NaN, and timed)
            say("  %-8s %-14s %5d %11.3e %9.2f %9.1f %9.1f %9.1f %9.1f %7.3f %11.3e"
                % (form, "%s %d" % (kind, h), width, cells, k["row_bytes"] / 1e9, k["rows_forward_ms"], k["rows_backward_ms"], k["edits_ms"], k["ms"], k["ms"] / k0["ms"],
                   nedit / (k["ms"] * 1e-3)))
            keep[vit, kind, h, width] = k["ms"]
            if vit and kind == "path" and h == 32 and width == 64:
                first = res[0]
for vit in (True, False):
    a, b = keep[vit, "path", 32, 64], keep[vit, "path", 32, 256]
    say("  %s, path band 32: 64 positions per workgroup %.1f ms, 256 %.1f ms: %d is the faster by %.1f %%"
        % ("viterbi" if vit else "forward", a, b, 64 if a < b else 256, 100.0 * abs(a - b) / max(a, b)))
edits = [("sub", i, c) for i in range(len(seqs[0])) for c in range(4)] + [("del", i, None) for i in range(len(seqs[0]))] + \
        [("ins", i, c) for i in range(len(seqs[0]) + 1) for c in range(4)]
flat = np.concatenate([np.ravel(first[1]), np.ravel(first[2]), np.ravel(first[3])])
top = [int(j) for j in np.argsort(-np.where(np.isnan(flat), -np.inf, flat), kind="stable")[:20]]
again = sa.map_post_to_sequences(sa.ScrappyMatrix.from_numpy(eng.posterior(sigs[0], MODEL), sloika=False),
                                 [text(sa.apply_edit(seqs[0], *edits[j])) for j in top], viterbi=True)
diff = flat[top].astype(np.float64) - again.astype(np.float64)
say("  read 0, its 20 highest edits in the path band of 32 scored again unbanded by k_map_pack: banded - unbanded between %.3g and %.3g on scores near %.1f (the edits and the exact engine add in different orders: rounding on either side)"
    % (float(diff.min()), float(diff.max()), float(first[0])))
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
