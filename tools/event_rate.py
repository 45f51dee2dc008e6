#!/usr/bin/env python3
"""Rate of event detection (scrappie_hip_detect_events_batch, csrc/sh_events.h), written to profiles/event_rate.txt: samples per
second for a batch of 4096 reads x 50 000 samples and for a batch of one read of 80 000 samples, and beside them the host
statement's single-thread rate on the same box (scrappie_hip_detect_events_host).  No figure is a gate: the single read is bound by
the serial walks (one lane sums, one lane detects) and may well be slower than the host.

    python tools/event_rate.py [--reads 4096] [--samples 50000] [--out profiles/event_rate.txt]
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
from scrappie_amd import synth  # noqa: E402


def batch(eng, reads, repeat):
    """(best wall seconds of the C call, its timing, events) over `repeat` calls after one warm-up"""
    n = len(reads)
    rts, keep = sa._raw_tables(reads)
    out = (sa._EventResult * n)()
    p = sa.DetectorParam()
    best, timing, nev = None, None, 0
    for it in range(repeat + 1):
        t0 = time.perf_counter()
        rc = sa.lib().scrappie_hip_detect_events_batch(eng._h, rts, n, C.byref(p), out)
        dt = time.perf_counter() - t0
        assert rc == 0, sa.last_error()
        nev = sum(out[i].events.n for i in range(n))
        sa.lib().scrappie_hip_free_event_results(out, n)
        if it and (best is None or dt < best):
            best, timing = dt, eng.event_timing()
    return best, timing, nev


def host(reads):
    t0 = time.perf_counter()
    for x in reads:
        sa.detect_events_host(x)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=50000)
    ap.add_argument("--single", type=int, default=80000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_rate.txt"))
    a = ap.parse_args()
    distinct = [synth.synthetic_signal(a.samples, 9000 + i, raw_units=True) for i in range(64)]
    reads = [distinct[i % 64] for i in range(a.reads)]
    one = [synth.synthetic_signal(a.single, 9100, raw_units=True)]
    eng = sa.Engine(0)
    lines = ["event detection: scrappie_hip_detect_events_batch (k_ev_sums, k_ev_tstat, k_ev_peaks, k_ev_events), best of %d calls after a warm-up" % a.repeat,
             "signals: synth.synthetic_signal(n, seed, raw_units=True); wall time of the C call (staging, upload, kernels, tables back, malloc per read)", ""]
    for name, rd in (("%d reads x %d samples" % (a.reads, a.samples), reads), ("1 read x %d samples" % a.single, one)):
        dt, tm, nev = batch(eng, rd, a.repeat)
        ns = sum(len(x) for x in rd)
        lines.append("%-28s %9.2f ms  %8.1f Msamples/s  (%d events; upload %.2f ms, kernels %.2f ms = %.1f Msamples/s, tables to the host %.2f ms)"
                     % (name, dt * 1e3, ns / dt / 1e6, nev, tm["upload_ms"], tm["detect_ms"], ns / tm["detect_ms"] / 1e3, tm["download_ms"]))
    hs = host(distinct[:16])
    lines.append("%-28s %9.2f ms  %8.1f Msamples/s  (one thread, 16 reads x %d samples)" % ("host statement", hs * 1e3, 16 * a.samples / hs / 1e6, a.samples))
    hs = host(one)
    lines.append("%-28s %9.2f ms  %8.1f Msamples/s  (one thread, 1 read x %d samples)" % ("host statement", hs * 1e3, a.single / hs / 1e6, a.single))
    eng.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
