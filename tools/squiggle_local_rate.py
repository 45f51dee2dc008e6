#!/usr/bin/env python3
"""Rate of mapping raw signals INTO a longer reference squiggle (scrappie_hip_squiggle_match_local_batch, k_squig_local; a DESIGN.md
record, not bench.py's `value`), and the measurement the default stride is chosen by.  Two shapes:
  a  2000 reads x 2000 samples into one shared reference of 50 000 positions, Viterbi scores, and with paths at the default
  b  16 reads x 4000 samples into one shared reference of 1 000 000 positions, Viterbi scores
Reads of these lengths are beyond the LDS home (a window holds at least 2 (samples - 1) + 1 cells, the home 1636): every window
keeps its rows in device scratch.  Strides of 1, 2, 4 and 8 entry positions per sample, and one window as the last resort (shape b:
measured once, without a warm-up).  The sample-bounded chunk loop the design allows is not built, so there is no on / off to
measure.  Every stride must give the same bits.  Best of `repeats` after a warm-up call, by the call's kernel time
(squiggle_timing's match_ms: the first pass), with the call's wall time beside it.  A DP cell is one position of one sample of
the reference, whatever the windows recompute.
The rule: the default is the fastest stride on shape a, provided it is within 3 % (the box-to-box spread the earlier profiles
record) of the fastest on shape b.
usage: squiggle_local_rate.py [repeats=2] [out=profiles/squiggle_local_rate.txt] [shapes=ab]"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scrappie_amd as sa
from scrappie_amd import synth

args = sys.argv[1:]
reps = int(args[0]) if len(args) > 0 else 2
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "squiggle_local_rate.txt")
which = args[2] if len(args) > 2 else "ab"
SPREAD = 0.03
MULS = (1, 2, 4, 8)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def make(L, nread, ns, seed):
    """a reference of L positions and nread windows of ns samples of its own simulated signal, each from another place"""
    params, sig, truth = synth.simulated_squiggle(L, seed, mean_dwell=8.0)
    rng = np.random.default_rng(seed)
    at = rng.integers(0, len(sig) - ns, nread)
    return params, [np.ascontiguousarray(sig[a:a + ns]) for a in at], [int(truth[a]) for a in at]


eng = sa.Engine(0)


def timed(fn, warm=True, n=None):
    if warm:
        fn()                                # warm-up: buffers and kernels at this shape
    best = None
    for _ in range(reps if n is None else n):
        t0 = time.perf_counter()
        r = fn()
        w = time.perf_counter() - t0
        t = eng.squiggle_timing()
        if best is None or t["match_ms"] < best[0]["match_ms"]:
            best = (t, w, r)
    return best


say("squiggle_local_rate: Viterbi, best kernel time of %d after a warm-up call; the LDS home ends at %d cells, the default stride is %d entry positions per sample"
    % (reps, sa.squiggle_local_max_cells(), int(sa.lib().scrappie_hip_squiggle_local_stride(10 ** 6, 4000, -1)) // 4000))
kernel_ms = {}
for name, (L, nread, ns) in (("a", (50000, 2000, 2000)), ("b", (1000000, 16, 4000))):
    if name not in which:
        continue
    params, sigs, truth = make(L, nread, ns, 11 if name == "a" else 12)
    cells = float(L) * ns * nread
    say("shape %s: %d reads x %d samples into one shared reference of %d positions (%.3e DP cells)" % (name, nread, ns, L, cells))
    want = None
    for mul in MULS + (0,):
        stride = mul * ns
        eng.debug_option("squig_local_stride", stride)
        pl = sa.squiggle_local_plan(L, ns, stride)
        last = mul == 0 and name == "b"
        t, w, res = timed(lambda: eng.match_squiggle_reference(sigs, params, viterbi=True, path=False), warm=not last, n=1 if last else None)
        got = np.array([r[0] for r in res], dtype=np.float32)
        assert np.all(np.isfinite(got))
        if want is None:
            want = got
            near = sum(1 for r, at in zip(res, truth) if abs(r[2] - 1 - at) <= 2 * ns)
            say("  (%d of %d reads end within 2 x %d positions of where their window of the simulated signal began)" % (near, nread, ns))
        assert got.tobytes() == want.tobytes(), (name, stride)
        kernel_ms[(name, mul)] = t["match_ms"]
        say("  %-34s %5d windows of %7d cells (%s): first pass %9.1f ms (%.3e cells/s), tables + uploads %7.1f ms, results %6.1f ms, wall %.3f s%s"
            % ("one window:" if mul == 0 else "stride %d x samples = %d:" % (mul, stride), len(pl["first"]), int(pl["ncell"].max()),
               "scratch" if pl["home"].all() else "LDS" if not pl["home"].any() else "both homes", t["match_ms"], cells / (t["match_ms"] * 1e-3), t["tables_ms"],
               t["walk_ms"], w, " (measured once, no warm-up)" if last else ""))
    eng.debug_option("squig_local_stride", -1)
    if name == "a":
        t, w, res = timed(lambda: eng.match_squiggle_reference(sigs, params, viterbi=True, path=True))
        assert np.array([r[0] for r in res], dtype=np.float32).tobytes() == want.tobytes()
        say("  the default stride with paths: first pass %.1f ms, second pass + walk + results %.1f ms, tables + uploads %.1f ms, wall %.3f s"
            % (t["match_ms"], t["walk_ms"], t["tables_ms"], w))
        t, w, res = timed(lambda: eng.match_squiggle_reference(sigs, params, viterbi=False))
        say("  the default stride, forward scores: first pass %.1f ms, wall %.3f s" % (t["match_ms"], w))

if "a" in which and "b" in which:
    every = MULS + (0,)
    label = lambda m: "one window" if m == 0 else "%d x samples" % m
    fast_b = min(kernel_ms[("b", m)] for m in every)
    ok = [m for m in every if kernel_ms[("b", m)] <= fast_b * (1 + SPREAD)]
    order = sorted(every, key=lambda m: kernel_ms[("a", m)])
    say("shape a, fastest first: %s" % ", ".join("%s %.1f ms" % (label(m), kernel_ms[("a", m)]) for m in order))
    say("within 3 %% of the fastest on shape b (%.1f ms): %s" % (fast_b, ", ".join(label(m) for m in ok)))
    both = [m for m in order if m in ok]
    if both:
        say("the rule's choice: %s%s" % (label(both[0]), "" if both[0] == order[0] else
            " (%+.1f %% behind %s on shape a, which is %+.0f %% behind on shape b)" % (100 * (kernel_ms[("a", both[0])] / kernel_ms[("a", order[0])] - 1), label(order[0]),
                                                                                    100 * (kernel_ms[("b", order[0])] / fast_b - 1))))
    else:
        say("the rule admits none")
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
