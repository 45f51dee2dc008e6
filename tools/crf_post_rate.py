#!/usr/bin/env python3
"""What base probabilities cost (k_crf_post, csrc/sh_crf_post.h), written to profiles/crf_post_rate.txt: samples per second of
Engine.basecall on rnnrf_r94-shaped synthetic weights without and with base_probs=True, the three terms of Engine.crf_post_timing() for the
latter (network + k_crf, k_crf_post, the probabilities' transfer), the host's posterior_crf (csrc/sh_host.c, libm, one thread) on the same
transitions, and the bytes that cross PCIe per read both ways.  No figure is a gate.

Every step that uses the GPU is a child process under a time limit of its own, and the steps are chained: the first one that fails, is
killed or runs out of time ends the run.

    python tools/crf_post_rate.py [--reads 10000] [--samples 4000] [--out profiles/crf_post_rate.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("plain", 300), ("probs", 300), ("host", 300))      # name, seconds


def best_of(fn, repeat):
    best = None
    for it in range(repeat + 1):              # (the first call warms up: arenas, code objects)
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if it and (best is None or dt < best):
            best = dt
    return best, out


def step(name, a):
    import scrappie_amd as sa
    from scrappie_amd import model, synth
    distinct = [synth.medmad_normalise(synth.synthetic_signal(a.samples, 9500 + i)) for i in range(32)]
    reads = [distinct[i % 32] for i in range(a.reads)]
    eng = sa.Engine(0)
    eng.load_model("rnnrf_r94", model.synthetic_model("rnnrf_r94", seed=11, size=96))
    res = {}
    if name == "plain":
        dt, calls = best_of(lambda: eng.basecall(reads, "rnnrf_r94"), a.repeat)
        res = {"seconds": dt, "nblock": sum(c["nblock"] for c in calls if c)}
    elif name == "probs":
        terms = []

        def run():
            out = eng.basecall(reads, "rnnrf_r94", base_probs=True)
            terms.append(eng.crf_post_timing())
            return out
        dt, calls = best_of(run, a.repeat)
        best = min(terms[1:], key=lambda t: sum(t.values()))
        res = {"seconds": dt, "nblock": sum(c["nblock"] for c in calls if c), "terms": best,
               "bytes_device": float(np.mean([c["base_probs"].size * 4 for c in calls if c]))}
    elif name == "host":
        trans = [sa.ScrappyMatrix.from_numpy(eng.posterior(x, "rnnrf_r94"), sloika=False) for x in distinct]
        t0 = time.perf_counter()
        for m in trans:
            sa.lib().free_scrappie_matrix(sa.lib().posterior_crf(m.data()))
        res = {"seconds": (time.perf_counter() - t0) * a.reads / len(trans),
               "bytes_host": float(np.mean([m.data().contents.nc * m.data().contents.stride * 4 for m in trans]))}
    eng.close()
    json.dump(res, open(a.json, "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crf_post_rate.txt"))
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    r = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            js = os.path.join(tmp, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reads", str(a.reads), "--samples", str(a.samples),
                                 "--repeat", str(a.repeat), "--step", name, "--json", js]).returncode
            if rc != 0:
                sys.exit("crf_post_rate: step '%s' ended with status %d; nothing further is run" % (name, rc))
            r[name] = json.load(open(js))
    nsamp = a.reads * a.samples
    tm = r["probs"]["terms"]
    lines = ["base probabilities of rnnrf_r94: Engine.basecall without and with base_probs=True, best of %d calls after a warm-up" % a.repeat,
             "%d reads x %d samples (32 distinct, synth.synthetic_signal), %d blocks; model.synthetic_model('rnnrf_r94', seed=11, size=96)" % (a.reads, a.samples, r["probs"]["nblock"]),
             "wall time of the Python call (signals staged from host memory, results unpacked into Python objects)", ""]
    for name, dt in (("basecall", r["plain"]["seconds"]), ("basecall(base_probs=True)", r["probs"]["seconds"])):
        lines.append("%-44s %9.2f ms  %8.3g samples/s" % (name, dt * 1e3, nsamp / dt))
    lines += ["", "Engine.crf_post_timing() of the fastest such call (device events, summed over its launch groups):"]
    for k, what in (("network_ms", "network + k_crf"), ("post_ms", "k_crf_post"), ("download_ms", "probabilities to the host (copy stream)")):
        lines.append("  %-42s %9.2f ms" % (what, tm[k]))
    lines += ["", "%-44s %9.2f ms  (csrc/sh_host.c through ctypes on the 32 distinct reads' transitions, one thread, scaled to %d)" % ("host posterior_crf, all reads", r["host"]["seconds"] * 1e3, a.reads),
              "%-44s %9.0f bytes a read (5 floats per block boundary)" % ("PCIe, base probabilities from the device", r["probs"]["bytes_device"]),
              "%-44s %9.0f bytes a read (the transition matrix, 28 floats per block, for the host to reduce)" % ("PCIe, per-read path", r["host"]["bytes_host"])]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
