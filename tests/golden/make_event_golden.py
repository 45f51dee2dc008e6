#!/usr/bin/env python3
"""Regenerate tests/golden/events/ref_event_detect.npz: the reference's event detection (src/event_detection.c), compiled here with the
flags of its Release build into a temporary directory, run on a fixed set of signals.  Needs /root/reference, gcc and the built
library of this repository (its fast5 reader gives the three bundled reads in pA).  The fixture is DATA only: inputs, the two
t-statistics of compute_tstat, and the event tables of detect_events.

Cases (key prefix; `cases` in the file lists those kept):
  synth_<n>     synth.synthetic_signal(n, seed = n, raw_units=True) for n = 11, 12, 13, 25, 500, 5000 (11: below twice the long window, so only the
                short detector sees anything)
  outlier       a 3000-sample synthetic read with sample 1500 set to 0.37 pA: one low outlier, which leaves every partial sum exact
  rounding      the case in which the sequential double sums do round: see rounding_case() below
  unordered     a 2000-sample synthetic read whose peaks come out of order, if a search of <= 2000 seeds finds one
  read_<name>   the three bundled reads in pA, whole (event tables only; inputs are tests/golden/fast5)
For every case the generator first runs the reference's own peak detector on its own t-statistics and keeps the case only if there
is a peak: with none, detect_events reads peaks[-1] and its result is undefined.  Dropped cases are listed under `dropped`.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import provenance  # noqa: E402
from scrappie_amd import synth  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "events", "ref_event_detect.npz")
# the fixture's own provenance record, in the format of tests/golden/PROVENANCE.json (which the other generators write and which stays
# as it is: this fixture lives in a folder of its own); tests/test_events_cpu.py::test_event_fixture_provenance checks it
RECORD = os.path.join(HERE, "events", "PROVENANCE.json")
SOURCES = ["src/event_detection.c", "src/event_detection.h", "src/scrappie_stdlib.h", "src/scrappie_structures.h", "reads/*.fast5"]


def write_record():
    import glob
    ref = {}
    for pat in SOURCES:
        for f in sorted(glob.glob(os.path.join(REF, pat))):
            ref[os.path.relpath(f, REF)] = provenance.sha(f)
    assert ref
    fixtures = {os.path.relpath(f, HERE): provenance.sha(f) for f in provenance.fixture_files("events/*.npz")}
    assert fixtures
    json.dump({"events/ref_event_detect.npz": {"fixtures": fixtures, "reference_files": ref}}, open(RECORD, "w"), indent=1, sort_keys=True)
    return RECORD
# CMakeLists.txt:97 (CMAKE_C_FLAGS_RELEASE)
RELEASE = ["-Wall", "-Wno-unused-function", "-fstack-protector-all", "-fgnu89-inline", "-O3", "-march=native", "-std=c99", "-DUSE_SSE2",
           "-D__USE_MISC", "-D_POSIX_SOURCE", "-DNDEBUG"]


class RawTable(C.Structure):
    _fields_ = [("uuid", C.c_char_p), ("n", C.c_size_t), ("start", C.c_size_t), ("end", C.c_size_t), ("raw", C.POINTER(C.c_float))]


class EventTable(C.Structure):
    _fields_ = [("n", C.c_size_t), ("start", C.c_size_t), ("end", C.c_size_t), ("event", C.c_void_p)]


class DetectorParam(C.Structure):
    _fields_ = [("window_length1", C.c_size_t), ("window_length2", C.c_size_t), ("threshold1", C.c_float), ("threshold2", C.c_float),
                ("peak_height", C.c_float)]


class Detector(C.Structure):          # event_detection.c:10-21 (layout only: the generator fills it as detect_events does)
    _fields_ = [("DEF_PEAK_POS", C.c_int), ("DEF_PEAK_VAL", C.c_float), ("signal", C.POINTER(C.c_float)), ("signal_length", C.c_size_t),
                ("threshold", C.c_float), ("window_length", C.c_size_t), ("masked_to", C.c_size_t), ("peak_pos", C.c_int),
                ("peak_value", C.c_float), ("valid_peak", C.c_bool)]


DEFAULTS = DetectorParam(3, 6, 1.4, 9.0, 0.2)
FLT_MAX = float(np.finfo(np.float32).max)


def build(tmp):
    so = os.path.join(tmp, "ref_event_detection.so")
    subprocess.run(["gcc"] + RELEASE + ["-fPIC", "-shared", "-I" + os.path.join(REF, "src"), os.path.join(REF, "src", "event_detection.c"), "-o", so, "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.compute_sum_sumsq.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_size_t]
    L.compute_sum_sumsq.restype = None
    L.compute_tstat.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_size_t, C.c_size_t]
    L.compute_tstat.restype = C.POINTER(C.c_float)
    L.short_long_peak_detector.argtypes = [C.POINTER(Detector), C.POINTER(Detector), C.c_float]
    L.short_long_peak_detector.restype = C.POINTER(C.c_size_t)
    L.detect_events.argtypes = [RawTable, DetectorParam]
    L.detect_events.restype = EventTable
    return L


libc = C.CDLL(None)
libc.free.argtypes = [C.c_void_p]


def reference(L, x):
    """(tstat1, tstat2, peaks in emission order, event table or None where there is no peak)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = len(x)
    xp = x.ctypes.data_as(C.POINTER(C.c_float))
    s, q = np.zeros(n + 1), np.zeros(n + 1)
    sp, qp = s.ctypes.data_as(C.POINTER(C.c_double)), q.ctypes.data_as(C.POINTER(C.c_double))
    L.compute_sum_sumsq(xp, sp, qp, n)
    t = []
    for w in (DEFAULTS.window_length1, DEFAULTS.window_length2):
        p = L.compute_tstat(sp, qp, n, w)
        t.append(np.ctypeslib.as_array(p, shape=(n,)).copy())
        libc.free(C.cast(p, C.c_void_p))
    det = [Detector(-1, FLT_MAX, t[k].ctypes.data_as(C.POINTER(C.c_float)), n, th, w, 0, -1, FLT_MAX, False)
           for k, (th, w) in enumerate(((DEFAULTS.threshold1, DEFAULTS.window_length1), (DEFAULTS.threshold2, DEFAULTS.window_length2)))]
    pk = L.short_long_peak_detector(C.byref(det[0]), C.byref(det[1]), DEFAULTS.peak_height)
    peaks = np.ctypeslib.as_array(pk, shape=(n,)).copy()
    libc.free(C.cast(pk, C.c_void_p))
    npeak = int(np.count_nonzero((peaks > 0) & (peaks < n)))
    assert np.all(peaks[npeak:] == 0)
    peaks = peaks[:npeak]
    if npeak == 0:
        return t[0], t[1], peaks, None, (s, q)
    et = L.detect_events(RawTable(None, n, 0, n, xp), DEFAULTS)
    assert et.event and et.n == npeak + 1 and et.start == 0 and et.end == et.n
    ev = np.ctypeslib.as_array(C.cast(et.event, C.POINTER(C.c_uint8)), shape=(et.n * synth.EVENT_DTYPE.itemsize,)).copy().view(synth.EVENT_DTYPE)
    libc.free(et.event)
    assert np.all(ev["pos"] == -1) and np.all(ev["state"] == -1)
    return t[0], t[1], peaks, ev, (s, q)


def tree_sums(v):
    """running sums of v (float64) in a tree order: sequential inside blocks of 64, block totals summed pairwise"""
    n = len(v)
    nb = (n + 63) // 64
    pad = np.zeros(nb * 64)
    pad[:n] = v
    inner = np.cumsum(pad.reshape(nb, 64), axis=1)
    tot = inner[:, -1].copy()
    # exclusive prefix of the block totals by recursive doubling
    pre = np.zeros(nb)
    inc = tot.copy()
    d = 1
    while d < nb:
        inc[d:] = inc[d:] + inc[:-d].copy()
        d *= 2
    pre[1:] = inc[:-1]
    return (inner + pre[:, None]).reshape(-1)[:n]


def rounds(x):
    """does some element of the running sums depend on the order of the additions?"""
    x = x.astype(np.float32)
    out = False
    for v in (x.astype(np.float64), (x * x).astype(np.float64)):
        out = out or bool(np.any(np.cumsum(v) != tree_sums(v)))
    return out


def outlier_case():
    x = synth.synthetic_signal(3000, 3000, raw_units=True)
    x[1500] = np.float32(0.37)
    return x


def rounding_case():
    """A read whose sequential double sums round, so that a scan in another order gives other bits.  The squares of a pA-scale read
    (~8e3 as floats: multiples of 2^-10) sum to ~2.4e7 over 3000 samples, where a double still resolves 2^-28; one sample of 0.37 pA
    (its square a multiple of 2^-26) leaves every partial sum exact, in any order: `outlier_rounds` in the file records that.  Here
    every seventh sample is a thousand times smaller (squares with bits down to 2^-43), and the partial sums round from the first of
    them on."""
    x = synth.synthetic_signal(3000, 3001, raw_units=True)
    x[10::7] *= np.float32(1e-3)
    return x


def main():
    sa = __import__("scrappie_amd")
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        cases = {}
        for n in (11, 12, 13, 25, 500, 5000):
            cases["synth_%d" % n] = synth.synthetic_signal(n, n, raw_units=True)
        cases["outlier"] = outlier_case()
        cases["rounding"] = rounding_case()
        assert rounds(cases["rounding"]), "the rounding case does not round"
        found = -1
        for seed in range(2000):
            x = synth.synthetic_signal(2000, 100000 + seed, raw_units=True)
            pk = reference(L, x)[2]
            if len(pk) > 1 and np.any(np.diff(pk.astype(np.int64)) < 0):
                cases["unordered"] = x
                found = 100000 + seed
                break
        # the bundled reads, whole, in pA
        lib = sa.lib()
        lib.scrappie_hip_read_raw.restype = sa._RawTable
        lib.scrappie_hip_read_raw.argtypes = [C.c_char_p, C.c_bool]
        reads = {}
        meta = json.load(open(os.path.join(HERE, "reads", "reads.json")))
        for name in sorted(meta):
            f = os.path.join(tmp, name + ".fast5")
            open(f, "wb").write(provenance.fixture_bytes(os.path.join(HERE, "fast5", name + ".fast5")))
            rt = lib.scrappie_hip_read_raw(os.fsencode(f), True)
            assert rt.raw and rt.n == meta[name]["n"]
            reads["read_" + name] = np.ctypeslib.as_array(rt.raw, shape=(rt.n,)).copy()
            sa._libc.free(C.cast(rt.raw, C.c_void_p))
        out, kept, dropped = {}, [], []
        for key, x in list(cases.items()) + list(reads.items()):
            t1, t2, pk, ev, _ = reference(L, x)
            if ev is None:
                dropped.append(key)
                continue
            kept.append(key)
            if key in cases:
                out[key + "__x"] = x
                out[key + "__tstat1"] = t1
                out[key + "__tstat2"] = t2
            for f in ("start", "length", "mean", "stdv"):
                out[key + "__" + f] = np.ascontiguousarray(ev[f])
        out["cases"] = np.array(kept)
        out["dropped"] = np.array(dropped, dtype="U32")
        out["unordered_seed"] = np.int64(found)                 # -1: the search found none
        out["outlier_rounds"] = np.bool_(rounds(cases["outlier"]))
        out["params"] = np.array([DEFAULTS.window_length1, DEFAULTS.window_length2, DEFAULTS.threshold1, DEFAULTS.threshold2, DEFAULTS.peak_height],
                                 dtype=np.float64)
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        np.savez_compressed(OUT, **out)
        provenance.split_large(OUT)
        print("kept", kept, "dropped", dropped, "unordered seed", found, "outlier rounds", bool(out["outlier_rounds"]))
    print(write_record())


if __name__ == "__main__":
    main()
