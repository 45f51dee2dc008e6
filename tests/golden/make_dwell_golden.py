#!/usr/bin/env python3
"""Regenerate tests/golden/dwell/ref_dwell.npz: the reference's dwell correction of homopolymer lengths (src/decode.c:511-702), as
oracle/_ref/libref_decode.so compiles it (`make -C oracle ref`; needs /root/reference), run on hand-made and seeded random paths.
The fixture is DATA only.  Per case <c> (listed in `cases`; `nstate_<c>` states):
  <c>__path      int32, an entry per event (-1: stay)
  <c>__start, <c>__length   the events' fields the correction reads (uint64, float32); dwell = (int)length
  <c>__plain, <c>__pos      overlapper's string and pos[]
  <c>__scales, <c>__dco     scales (float32) and dwell_corrected_overlapper's strings at them, dwell = (int)length
  <c>__corrected            homopolymer_dwell_correction's string, the events annotated with pos and state = 1 + path
  <c>__scale_bits           its homo_scale as float bits: recomputed here in numpy float32 / float64 in the reference's order, and
                            asserted to give the reference's string through dwell_corrected_overlapper
Strings are what strlen sees: a call that ends inside a homopolymer with bases to add is one character short of the reference's own
`length` (decode.c:633-635).  No path is all stays: the reference is undefined there.

Hand-made cases (1025 states): the worked examples of decode.c's behaviour (a first k-mer that is a homopolymer is none; a path that
ends inside one, with and without bases to add), a homopolymer broken by stays, two homopolymers in direct succession, leading stays,
a single k-mer, no step at all (the scale is the prior alone), dwell / scale of exactly x.5 for odd and even x, and a read whose
corrected call is longer than the 5 (T + 1) + 16 bytes a plain call may need.  Random cases: walks biased towards homopolymer k-mers,
about 40 % stays, geometric dwells of mean 9, path lengths around the eight-wide unroll of the device's loads; 1025 states, and 65.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import provenance  # noqa: E402
from scrappie_amd import synth  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "dwell", "ref_dwell.npz")
RECORD = os.path.join(HERE, "dwell", "PROVENANCE.json")
SOURCES = ["src/decode.c", "src/decode.h", "src/util.c", "src/util.h", "src/sse_mathfun.h", "src/scrappie_matrix.h", "src/scrappie_structures.h"]
LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 300)
f32, f64 = np.float32, np.float64


class EventTable(C.Structure):
    _fields_ = [("n", C.c_size_t), ("start", C.c_size_t), ("end", C.c_size_t), ("event", C.c_void_p)]


class DwellModel(C.Structure):
    _fields_ = [("scale", C.c_float), ("base_adj", C.c_float * 4)]


ip = C.POINTER(C.c_int)
libc = C.CDLL(None)
libc.free.argtypes = [C.c_void_p]


def load():
    L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_decode.so"))
    L.overlapper.restype = C.c_void_p
    L.overlapper.argtypes = [ip, C.c_size_t, C.c_int, ip]
    L.dwell_corrected_overlapper.restype = C.c_void_p
    L.dwell_corrected_overlapper.argtypes = [ip, ip, C.c_int, C.c_int, DwellModel]
    L.homopolymer_dwell_correction.restype = C.c_void_p
    L.homopolymer_dwell_correction.argtypes = [EventTable, ip, C.c_size_t, C.c_size_t]
    return L


def take(p):
    assert p
    s = C.string_at(p).decode()
    libc.free(p)
    return s


def kmer(s):
    v = 0
    for ch in s:
        v = v * 4 + "ACGT".index(ch)
    return v


def path_of(*names):
    return np.array([-1 if x is None else kmer(x) for x in names], dtype=np.int32)


def events_of(dwell):
    """contiguous events of these lengths (whole samples, as detect_events makes them)"""
    ev = np.zeros(len(dwell), dtype=synth.EVENT_DTYPE)
    ev["length"] = np.asarray(dwell, dtype=f32)
    ev["start"] = np.concatenate(([0], np.cumsum(np.asarray(dwell, dtype=np.uint64))[:-1]))
    ev["mean"], ev["stdv"], ev["pos"], ev["state"] = 80.0, 1.0, -1, -1
    return ev


def numpy_scale(ev, pos, path, basecall_len):
    """decode.c:666-693 in numpy: int sums, a float32 division and addition, a float64 division rounded to float32 once"""
    dwell = ev["length"].astype(np.int32)
    tot, nstep, ppos, evdwell, pstate = 0, 0, -2, 0, -1
    for k in range(len(ev)):
        if pos[k] == ppos:
            evdwell += int(dwell[k])
            continue
        if pos[k] == ppos + 1 and 1 + int(path[k]) != pstate:
            tot += evdwell
            nstep += 1
        evdwell, ppos, pstate = int(dwell[k]), int(pos[k]), 1 + int(path[k])
    start_delta = f32(int(ev["start"][-1]) - int(ev["start"][0]))
    prior = f32(f32(ev["length"][-1] + start_delta) / f32(basecall_len))
    num = f32(prior + f32(tot))
    return f32(f64(num) / (f64(1.0) + f64(nstep))), tot, nstep


def reference(L, path, ev, nstate, scales=()):
    path = np.ascontiguousarray(path, dtype=np.int32)
    n = len(path)
    assert n == len(ev) and np.any(path >= 0)
    pos = np.zeros(n, dtype=np.int32)
    plain = take(L.overlapper(path.ctypes.data_as(ip), n, nstate - 1, pos.ctypes.data_as(ip)))
    ann = ev.copy()
    ann["pos"], ann["state"] = pos, path + 1
    et = EventTable(n, 0, n, ann.ctypes.data)
    corrected = take(L.homopolymer_dwell_correction(et, path.ctypes.data_as(ip), nstate, len(plain)))
    dwell = np.ascontiguousarray(ev["length"].astype(np.int32))
    dco = lambda s: take(L.dwell_corrected_overlapper(path.ctypes.data_as(ip), dwell.ctypes.data_as(ip), n, nstate - 1,
                                                      DwellModel(float(s), (C.c_float * 4)(0, 0, 0, 0))))
    scale, tot, nstep = numpy_scale(ann, pos, path, len(plain))
    assert dco(scale) == corrected, "the recomputed scale does not reproduce the reference's string"
    return dict(path=path, start=ev["start"].copy(), length=ev["length"].copy(), plain=np.array(plain), pos=pos,
                scales=np.array(scales, dtype=f32), dco=np.array([dco(s) for s in scales], dtype="U"),
                corrected=np.array(corrected), scale_bits=np.array(scale).view(np.uint32)), (scale, tot, nstep)


def random_path(rng, n, klen):
    """a walk biased towards homopolymer k-mers; about 40 % stays; never all stays"""
    nk = 4 ** klen
    homo = lambda k: all(((k >> (2 * i)) & 3) == (k & 3) for i in range(klen))
    path = np.full(n, -1, dtype=np.int32)
    cur = None
    for k in range(n):
        if rng.random() < 0.4:
            continue
        if cur is None:
            cur = int(rng.integers(nk)) if rng.random() < 0.8 else (nk - 1) // 3 * int(rng.integers(4))
        elif homo(cur) and rng.random() < 0.45:
            pass                                            # the homopolymer's k-mer again
        else:
            for _ in range(2 if rng.random() < 0.05 else 1):     # a step, seldom a skip
                b = (cur & 3) if rng.random() < 0.7 else int(rng.integers(4))
                cur = ((cur << 2) | b) & (nk - 1)
        path[k] = cur
    if not np.any(path >= 0):
        path[int(rng.integers(n))] = int(rng.integers(nk))
    return path


def half_cases(L):
    """dwells for a fixed path, searched so that the LAST homopolymer dwell over homo_scale is exactly x.5 in float, x odd and x even"""
    path = path_of("ACGTA", "CGTAA", "GTAAA", "TAAAA", "AAAAA", None, "AAAAA", "AAAAC", "AAACG")
    rng = np.random.default_rng(505)
    found = {}
    for _ in range(200000):
        dwell = rng.integers(1, 40, size=len(path))
        _, (scale, _, _) = reference(L, path, events_of(dwell), 1025)
        q = f32(f32(int(dwell[4:7].sum())) / scale)
        if q % 1 == f32(0.5) and q > 1:
            found.setdefault("odd" if int(q) % 2 else "even", dwell)
            if len(found) == 2:
                return path, found
    raise AssertionError("no dwells with an exact half found")


def write_record():
    import glob
    ref = {}
    for pat in SOURCES:
        for f in sorted(glob.glob(os.path.join(REF, pat))):
            ref[os.path.relpath(f, REF)] = provenance.sha(f)
    assert ref
    fixtures = {os.path.relpath(f, HERE): provenance.sha(f) for f in provenance.fixture_files("dwell/*.npz")}
    assert fixtures
    json.dump({"dwell/ref_dwell.npz": {"fixtures": fixtures, "reference_files": ref}}, open(RECORD, "w"), indent=1, sort_keys=True)
    return RECORD


def main():
    L = load()
    cases, nstates = {}, {}

    def add(name, path, dwell, nstate=1025, scales=(), want=None):
        c, info = reference(L, path, events_of(dwell), nstate, scales)
        if want is not None:
            assert list(c["dco"]) == list(want), (name, list(c["dco"]), want)
        cases[name], nstates[name] = c, nstate
        return c, info

    # the worked examples
    add("first_homo", path_of("AAAAA", None, "AAAAA", "AAAAC"), [10] * 4, scales=[10.0], want=["AAAAAAAC"])
    seven = path_of("ACGTA", "CGTAA", "GTAAA", "TAAAA", "AAAAA", None, "AAAAA")
    add("ends_inside", seven, [10] * 7, scales=[10.0], want=["ACGTAAAAAAA"])
    add("ends_inside_zero", seven, [10, 10, 10, 10, 2, 1, 1], scales=[10.0], want=["ACGTAAAAA"])
    add("first_homo_stays", path_of("AAAAA", None, None, "AAAAC"), [10, 30, 30, 10], scales=[10.0], want=["AAAAAC"])
    add("broken_by_stays", path_of("ACGTT", "CGTTT", "GTTTT", "TTTTT", None, None, "TTTTT", None, "TTTTT", "TTTTA", "TTTAC"),
        [8, 9, 7, 12, 20, 3, 9, 14, 6, 8, 9], scales=[9.0, 3.0])
    add("two_in_succession", path_of("GCAAA", "CAAAA", "AAAAA", None, "CCCCC", None, "CCCCG", "CCCGT"), [9, 8, 25, 11, 31, 17, 9, 8], scales=[9.0, 4.0])
    add("leading_stays", path_of(None, None, None, "ACGGG", "CGGGG", "GGGGG", None, "GGGGT"), [5, 6, 7, 9, 8, 20, 19, 9], scales=[9.0])
    c, (s, tot, nstep) = add("one_kmer", path_of(None, "ACGTA", None, None), [7, 9, 11, 5], scales=[9.0])
    assert nstep == 0
    c, (s, tot, nstep) = add("no_step", path_of("AAAAA", "AAAAA", None, "AAAAA"), [6, 13, 9, 14], scales=[6.0])
    assert nstep == 0 and tot == 0 and c["corrected"] != c["plain"]
    hpath, found = half_cases(L)
    for kind, dwell in sorted(found.items()):
        add("half_" + kind, hpath, dwell, scales=[4.0, 8.0])
    # dwell_corrected_overlapper alone at exact halves: 10 / 4 = 2.5 -> 3, 14 / 4 = 3.5 -> 4 (half away from zero, not to even)
    add("half_scales", path_of("ACGTA", "CGTAA", "GTAAA", "TAAAA", "AAAAA", "AAAAC"), [4, 4, 4, 4, 10, 4], scales=[4.0], want=["ACGT" + 8 * "A" + "C"])
    add("half_scales_odd", path_of("ACGTA", "CGTAA", "GTAAA", "TAAAA", "AAAAA", "AAAAC"), [4, 4, 4, 4, 14, 4], scales=[4.0], want=["ACGT" + 9 * "A" + "C"])
    # longer than a plain call's reservation: 8 entries, 5 * 8 + 16 = 56 bytes (64 rounded up to 16)
    # (a dwell that a later step counts enters the scale and limits itself: the long one is the path's last, seven short steps before it)
    long_path = path_of("ACGTC", "CGTCG", "GTCGT", "TCGTA", "CGTAA", "GTAAA", "TAAAA", "AAAAA")
    for h in range(10, 4000, 10):
        c, _ = reference(L, long_path, events_of([2] * 7 + [h]), 1025)
        if 70 <= len(str(c["corrected"])) <= 90:
            add("over_long", long_path, [2] * 7 + [h])
            break
    assert "over_long" in cases

    nrand = ndiff = 0
    for nstate, klen, seeds in ((1025, 5, 10), (65, 3, 2)):
        for n in LENGTHS:
            for seed in range(seeds):
                rng = np.random.default_rng([nstate, n, seed])
                path = random_path(rng, n, klen)
                c, _ = add("rand%d_%d_%d" % (nstate, n, seed), path, rng.geometric(1.0 / 9.0, size=n), nstate, scales=[9.0])
                nrand += 1
                ndiff += bool(c["corrected"] != c["plain"])
    assert 2 * ndiff >= nrand, "only %d of %d random cases are changed by the correction: the fixture would test nothing" % (ndiff, nrand)

    out = {"cases": np.array(sorted(cases))}
    for name, c in cases.items():
        out["nstate_" + name] = np.int32(nstates[name])
        for k, v in c.items():
            out[name + "__" + k] = v
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    provenance.split_large(OUT)
    print("%d cases (%d of 1025 states); the correction changes %d of %d random ones; %d bytes" %
          (len(cases), sum(1 for v in nstates.values() if v == 1025), ndiff, nrand, os.path.getsize(OUT) if os.path.exists(OUT) else -1))
    print(write_record())


if __name__ == "__main__":
    main()
