#!/usr/bin/env python3
"""Rate of events basecalling (scrappie_hip_basecall_events_batch: detection, features on host threads, the events model, the stitching),
written to profiles/events_call_rate.txt: events per second of Engine.basecall_events with the dwell correction on the device
(dwell=True), without it (dwell=False), and without it followed by the host statement of the correction
(homopolymer_dwell_correction, csrc/sh_host.c) for every read on one thread -- what the correction would cost on the host, the path
already there.  No figure is a gate.  The model is model.homopolymer_cycle_model(): its calls have homopolymers for the correction to
work on.

    python tools/events_call_rate.py [--reads 2048] [--samples 20000] [--out profiles/events_call_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scrappie_amd as sa  # noqa: E402
from scrappie_amd import model, synth  # noqa: E402


def best_of(fn, repeat):
    best = None
    for it in range(repeat + 1):              # (the first call warms up: arenas, code objects)
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if it and (best is None or dt < best):
            best = dt
    return best, out


def host_inputs(eng, x):
    """what the host statement takes for one read: annotated events, the path, the plain call's length (None: no call)"""
    ev = eng.detect_events([x])[0]
    if ev is None:
        return None
    post = eng.posterior(sa.event_features(ev).ravel(), "nanonet_events")
    pm = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    n = len(ev)
    ip = C.POINTER(C.c_int)
    path, pos = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    sa.lib().decode_transducer(pm.data(), 0.0, 0.0, 2.0, path.ctypes.data_as(ip), False)
    plain = sa._take_string(sa.lib().overlapper(path.ctypes.data_as(ip), n + 1, post.shape[1] - 1, pos.ctypes.data_as(ip)))
    if plain is None:
        return None
    ev["pos"], ev["state"] = pos[:n], path[:n] + 1
    return ev, path, post.shape[1], len(plain)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_call_rate.txt"))
    a = ap.parse_args()
    distinct = [synth.synthetic_signal(a.samples, 9300 + i, raw_units=True) for i in range(32)]
    reads = [distinct[i % 32] for i in range(a.reads)]
    eng = sa.Engine(0)
    eng.load_model("nanonet_events", model.homopolymer_cycle_model())
    t_on, calls_on = best_of(lambda: eng.basecall_events(reads, "nanonet_events", dwell=True), a.repeat)
    t_off, calls_off = best_of(lambda: eng.basecall_events(reads, "nanonet_events", dwell=False), a.repeat)
    nev = sum(c["nblock"] for c in calls_on if c)
    changed = sum(1 for x, y in zip(calls_on, calls_off) if x and y and x["bases"] != y["bases"])
    inputs = [host_inputs(eng, x) for x in distinct]
    t0 = time.perf_counter()
    for inp in inputs:
        if inp is not None:
            sa.homopolymer_dwell_correction(*inp)
    t_host = (time.perf_counter() - t0) * a.reads / len(distinct)
    redo = int(eng.debug_fetch("n_redo", np.uint64)[0])
    eng.close()
    lines = ["events basecalling: Engine.basecall_events (scrappie_hip_basecall_events_batch with dwell=True), best of %d calls after a warm-up" % a.repeat,
             "%d reads x %d samples (32 distinct, synth.synthetic_signal(n, seed, raw_units=True)), %d events; model.homopolymer_cycle_model()" % (a.reads, a.samples, nev),
             "wall time of the Python call; the correction changes %d of %d calls; reads left to the host: %d" % (changed, a.reads, redo), ""]
    for name, dt in (("dwell=True (on the device)", t_on), ("dwell=False", t_off), ("dwell=False + host statement, one thread", t_off + t_host)):
        lines.append("%-42s %9.2f ms  %8.2f Mevents/s" % (name, dt * 1e3, nev / dt / 1e6))
    lines.append("%-42s %9.2f ms  (homopolymer_dwell_correction through ctypes, the 32 distinct reads scaled to %d)" % ("host statement alone, one thread", t_host * 1e3, a.reads))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
