#!/usr/bin/env python3
"""Rate of scoring every single-base edit of a sequence for a transducer model (scrappie_hip_map_edits_batch; a DESIGN.md record, not
bench.py's `value`).  10 000 synthetic reads of 4000 samples (800 blocks, synthetic rgrgr_r94 weights), each against its own call
-- or, where the synthetic weights call it in fewer than 8 bases, a random sequence of a third of its blocks in bases --, Viterbi and
forward.  Best wall of `repeats` after a warm-up call, with scrappie_hip_map_timing's split of that call and
scrappie_hip_map_edits_timing's: the three kernels by events on the stream, the launches the cut made and their row bytes.  In the
same process, for the yardstick: the same reads against that sequence and 7 edits of it through scrappie_hip_map_multi_batch
(k_map_pack at its default) -- its kernel time per candidate is what scoring ONE edit cost before this call existed; the time for
all 9 L + 4 is that price EXTRAPOLATED, a run that was never made -- and 20 of the edits the call scores highest on the first read
scored again by that engine.
usage: map_edits_rate.py [reads=10000] [samples=4000] [repeats=2] [out=profiles/map_edits_rate.txt]"""
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
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "map_edits_rate.txt")
MODEL = "rgrgr_r94"
rng = np.random.default_rng(1)
long_sig = synth.medmad_normalise(synth.synthetic_signal(ns + 64 * 7, 5))
sigs = [long_sig[(i % 64) * 7:(i % 64) * 7 + ns].copy() for i in range(n)]      # every read a different window of one signal
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def text(codes):
    return "".join("ACGT"[b] for b in codes)


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
eng.load_model(MODEL, model.synthetic_model(MODEL, seed=1))
nblock = eng.read_blocks(MODEL, ns)
maxL = int(sa.lib().scrappie_hip_map_edits_max_bases(5))
calls = {}
for i in range(min(n, 64)):                  # the reads are 64 windows of one signal: 64 calls
    c = eng.basecall([sigs[i]], MODEL)[0]
    b = c["bases"] if c is not None and len(c["bases"]) >= 8 else "".join(rng.choice(list("ACGT"), max(8, nblock // 3)))
    calls[i] = sa.encode_bases(b[:maxL], 1).astype(np.int32)
seqs = [calls[i % 64] for i in range(n)]
nedit = sum(9 * len(s) + 4 for s in seqs)
row_bytes = sum(int(sa.lib().scrappie_hip_map_edits_row_bytes(len(s), 5, nblock)) for s in seqs)
say("map_edits_rate: %d reads of %d samples (%d blocks), each against its sequence (%.0f bases on average): %.3e edits, %.2f GB of rows; best wall of %d after a warm-up call"
    % (n, ns, nblock, sum(len(s) for s in seqs) / float(n), nedit, row_bytes / 1e9, reps))
kernel_ms = {}
for vit in (True, False):
    w, walls, (sp, k), res = timed(lambda: eng.score_edits_transducer(sigs, seqs, model=MODEL, viterbi=vit), lambda: (eng.map_timing(), eng.map_edits_timing()))
    ks = k["rows_forward_ms"] + k["rows_backward_ms"] + k["edits_ms"]
    kernel_ms[vit] = ks
    assert all(np.isfinite(r[0]) for r in res[:64]) and k["row_bytes"] == row_bytes
    say("  %s wall %.3f s (%s); network + S1 %.1f ms, the three launches with their copies %.1f ms"
        % ("viterbi:" if vit else "forward:", w, ", ".join("%.3f" % x for x in walls), sp["network_ms"], sp["map_ms"]))
    say("           k_map_edits_rows forward %.1f ms, backward %.1f ms, k_map_edits %.1f ms: %.1f ms in the kernels, %.3e edits/s; %d launch(es), %.2f GB of rows written, %.2f GB/s over k_map_edits' six loads per (position, block)"
        % (k["rows_forward_ms"], k["rows_backward_ms"], k["edits_ms"], ks, nedit / (ks * 1e-3), k["launches"], k["row_bytes"] / 1e9,
           3.0 * k["row_bytes"] / 1e9 / (k["edits_ms"] * 1e-3)))
    if vit:
        first = res[0]

# the yardstick: the sequence and 7 edits of it per read through k_map_pack
edits = [("sub", i, c) for i in range(len(seqs[0])) for c in range(4)] + [("del", i, None) for i in range(len(seqs[0]))] + \
        [("ins", i, c) for i in range(len(seqs[0]) + 1) for c in range(4)]
flat = np.concatenate([np.ravel(first[1]), np.ravel(first[2]), np.ravel(first[3])])
pick7 = [int(x) for x in rng.choice(len(edits), 7, replace=False)]
lists = [[text(seqs[i])] + [text(sa.apply_edit(seqs[i], kind, min(p, len(seqs[i]) - 1), c)) for kind, p, c in (edits[j] for j in pick7)] for i in range(min(n, 64))]
lists = [lists[i % 64] for i in range(n)]
w, walls, sp, res = timed(lambda: eng.map_to_sequences(sigs, lists, model=MODEL, viterbi=True, path=False), eng.map_timing)
per_cand = sp["map_ms"] / (8.0 * n)
say("  yardstick, the sequence and 7 edits per read through k_map_pack: wall %.3f s; network + S1 %.1f ms, k_map_pack %.1f ms: %.3e ms per candidate, %.3e edits/s"
    % (w, sp["network_ms"], sp["map_ms"], per_cand, 1.0 / (per_cand * 1e-3)))
say("  all %.3e edits at that price (an EXTRAPOLATION, never run): %.1f s; the three kernels: viterbi %.3f s -- %.1fx; forward %.3f s -- %.1fx"
    % (nedit, nedit * per_cand * 1e-3, kernel_ms[True] * 1e-3, nedit * per_cand / kernel_ms[True], kernel_ms[False] * 1e-3, nedit * per_cand / kernel_ms[False]))
top = [int(j) for j in np.argsort(-np.where(np.isnan(flat), -np.inf, flat), kind="stable")[:20]]
again = sa.map_post_to_sequences(sa.ScrappyMatrix.from_numpy(eng.posterior(sigs[0], MODEL), sloika=False),
                                 [text(sa.apply_edit(seqs[0], *edits[j])) for j in top], viterbi=True)
diff = np.abs(flat[top].astype(np.float64) - again.astype(np.float64))
say("  read 0, its 20 highest edits scored again by k_map_pack: largest |difference| %.3g on scores near %.1f (%.2g relative)"
    % (float(diff.max()), float(first[0]), float(diff.max()) / abs(float(first[0]))))
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
