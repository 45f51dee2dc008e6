#!/usr/bin/env python3
"""Rate of matching one signal to many candidate squiggles (scrappie_hip_squiggle_match_multi_batch; a DESIGN.md record, not
bench.py's `value`), and the measurement the default pack size is chosen by.  Viterbi scores, two shapes:
  a  2000 reads x 3000 samples against 24 shared candidates of 40 positions (barcodes)
  b  300 reads x 3000 samples against 8 candidates of ~400 positions per read: a squiggle of the read's own and 7 edits of it
and three routes:
  (i)   Engine.match_squiggle with every read repeated once per candidate -- the only way before this call existed.  With
        `baseline` as the first argument ONLY this route runs, and the record is appended to: that is how the parent commit
        is measured, from a checkout of it with this file copied into its tools/
  (ii)  squig_pack_cells = 0: the signal once per pair still, k_squig per candidate, one workgroup each
  (iii) packed: k_squig_pack at pack_cells 128, 256, 512, 1024 and the most a pack holds (1024 is more than that and counts as
        the most).  A candidate that is alone in its pack takes k_squig; shape b, where every candidate is, is also measured
        with the debug option squig_pack_lone, which keeps such a candidate in k_squig_pack
Every route must give the same bits.  Best of `repeats` after a warm-up call, by the call's kernel time (squiggle_timing's
match_ms), with the call's wall time beside it.
The rule: the default is the fastest of (iii) on shape a that is not slower on shape b than (ii) by more than 3 % (the
box-to-box spread, README); if no packed setting beats (ii) on shape a, packing does not pay.
usage: squiggle_pack_rate.py [baseline] [repeats=2] [out=profiles/squiggle_pack_rate.txt]"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scrappie_amd as sa
from scrappie_amd import synth

args = sys.argv[1:]
baseline = bool(args) and args[0] == "baseline"
if baseline:
    args = args[1:]
reps = int(args[0]) if len(args) > 0 else 2
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "squiggle_pack_rate.txt")
SPREAD = 0.03
NS = 3000
rng = np.random.default_rng(1)


def edit(params):
    """a few substituted positions, a deletion and an insertion"""
    p = params.copy()
    for _ in range(3):
        p[int(rng.integers(len(p))), 0] += np.float32(rng.normal(0.0, 1.0))
    if rng.random() < 0.5:
        p = np.delete(p, int(rng.integers(len(p))), axis=0)
    if rng.random() < 0.5:
        at = int(rng.integers(len(p)))
        p = np.insert(p, at, p[at], axis=0)
    return np.ascontiguousarray(p, dtype=np.float32)


def window(sig, i):
    """NS samples of a simulated signal, tiled where it is shorter"""
    if len(sig) < NS + 64:
        sig = np.tile(sig, (NS + 64) // len(sig) + 1)
    return np.ascontiguousarray(sig[i % 64:i % 64 + NS])


barcodes = [synth.simulated_squiggle(40, 100 + k)[0] for k in range(24)]
own_a = [synth.simulated_squiggle(400, 200 + k) for k in range(8)]
sig_a = [window(own_a[i % 8][1], i) for i in range(2000)]
own_b = [synth.simulated_squiggle(400, 300 + k) for k in range(16)]
sig_b = [window(own_b[i % 16][1], i) for i in range(300)]
cand_b = [[own_b[i % 16][0]] + [edit(own_b[i % 16][0]) for _ in range(7)] for i in range(300)]
shapes = {"a": (sig_a, [barcodes] * 2000, barcodes, "2000 reads x 3000 samples, 24 shared candidates of 40 positions"),
          "b": (sig_b, cand_b, cand_b, "300 reads x 3000 samples, 8 candidates of ~400 positions per read")}

eng = sa.Engine(0)
maxc = sa.squiggle_pack_max_cells() if hasattr(sa, "squiggle_pack_max_cells") else 0
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn):
    fn()                                    # warm-up: buffers and kernels at this shape
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        w = time.perf_counter() - t0
        t = eng.squiggle_timing()
        if best is None or t["match_ms"] < best[0]["match_ms"]:
            best = (t, w, r)
    return best


say("squiggle_pack_rate%s: Viterbi scores, best kernel time of %d after a warm-up call%s"
    % (" (route (i) only: the parent commit's build)" if baseline else "", reps,
       "" if baseline else "; a pack holds at most %d cells" % maxc))
kernel_ms = {}
for name, (sigs, lists, arg, what) in shapes.items():
    cells = float(NS) * sum(len(q) for c in lists for q in c)
    say("shape %s: %s (%.3e DP cells)" % (name, what, cells))
    flat_s = [x for x, c in zip(sigs, lists) for _ in c]
    flat_q = [q for c in lists for q in c]
    t, w, res = timed(lambda: eng.match_squiggle(flat_s, flat_q, viterbi=True, path=False))
    want = np.array([s for s, _ in res], dtype=np.float32)
    assert np.all(np.isfinite(want))
    kernel_ms[(name, "i")] = t["match_ms"]
    say("  (i)   every read repeated per candidate:    k_squig %8.1f ms (%.3e cells/s), tables + uploads %7.1f ms, results %5.1f ms, wall %.3f s"
        % (t["match_ms"], cells / (t["match_ms"] * 1e-3), t["tables_ms"], t["walk_ms"], w))
    del flat_s, flat_q, res
    if baseline:
        continue
    for pc in (0, 128, 256, 512, 1024, maxc):
        eng.debug_option("squig_pack_cells", pc)
        t, w, res = timed(lambda: eng.match_squiggles(sigs, arg, viterbi=True, path=False))
        got = np.concatenate([sc for sc, _, _ in res])
        assert got.tobytes() == want.tobytes(), (name, pc)
        kernel_ms[(name, pc)] = t["match_ms"]
        say("  %s %8.1f ms (%.3e cells/s), tables + uploads %7.1f ms, results %5.1f ms, wall %.3f s"
            % ("(ii)  k_squig per candidate (pack_cells 0):  k_squig     " if pc == 0 else "(iii) packed, pack_cells %4d:               kernels     " % pc,
               t["match_ms"], cells / (t["match_ms"] * 1e-3), t["tables_ms"], t["walk_ms"], w))
    if name == "b":
        eng.debug_option("squig_pack_lone", 1)
        for pc in (128, maxc):
            eng.debug_option("squig_pack_cells", pc)
            t, w, res = timed(lambda: eng.match_squiggles(sigs, arg, viterbi=True, path=False))
            assert np.concatenate([sc for sc, _, _ in res]).tobytes() == want.tobytes(), (name, pc, "lone")
            say("  (iii) with squig_pack_lone, pack_cells %4d:  k_squig_pack %8.1f ms (%.3e cells/s), tables + uploads %7.1f ms, results %5.1f ms, wall %.3f s"
                % (pc, t["match_ms"], cells / (t["match_ms"] * 1e-3), t["tables_ms"], t["walk_ms"], w))
        eng.debug_option("squig_pack_lone", 0)
    eng.debug_option("squig_pack_cells", -1)
    t, w, res = timed(lambda: eng.match_squiggles(sigs, arg, viterbi=True, path=True))
    say("  the default with the best candidate's path: kernels %.1f ms, tables + uploads %.1f ms, walk + results %.1f ms, wall %.3f s"
        % (t["match_ms"], t["tables_ms"], t["walk_ms"], w))

if not baseline:
    for name in shapes:
        d = kernel_ms[(name, 0)] / kernel_ms[(name, "i")] - 1.0
        say("shape %s: pack_cells 0 against route (i) of this build, kernel time: %+.1f %% (%s the 3 %% spread)" % (name, 100 * d, "within" if abs(d) <= SPREAD else "OUTSIDE"))
    packed = (128, 256, 512, 1024, maxc)
    ok = [pc for pc in packed if kernel_ms[("b", pc)] <= kernel_ms[("b", 0)] * (1 + SPREAD)]
    say("packed settings not slower than (ii) on shape b by more than 3 %%: %s" % (ok or "none"))
    if ok:
        order = sorted(ok, key=lambda pc: kernel_ms[("a", pc)])
        pick = order[0]
        gain = kernel_ms[("a", 0)] / kernel_ms[("a", pick)]
        say("fastest of them on shape a: pack_cells %d, %.1f ms against %.1f ms for (ii): %.2fx -- %s%s"
            % (pick, kernel_ms[("a", pick)], kernel_ms[("a", 0)], gain, "packing pays" if gain > 1 else "NO packed setting beats k_squig per candidate",
               "; the runner-up, pack_cells %d, is %.1f %% behind" % (order[1], 100 * (kernel_ms[("a", order[1])] / kernel_ms[("a", pick)] - 1)) if len(order) > 1 else ""))
    else:
        best = min(packed, key=lambda pc: kernel_ms[("a", pc)])
        say("the rule admits none; the fastest packed setting on shape a is pack_cells %d: %.1f ms against %.1f ms for (ii)" % (best, kernel_ms[("a", best)], kernel_ms[("a", 0)]))
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if baseline else "w") as fh:
    fh.write("\n".join(lines) + "\n")
