"""The dwell correction of homopolymer lengths on the host (csrc/sh_host.c: homopolymer_dwell_correction, dwell_corrected_overlapper),
no GPU: the statements the kernels of sh_dwell.h are held against equal the reference's decode.c on every case of
tests/golden/dwell/ref_dwell.npz (tests/golden/make_dwell_golden.py) -- strings as strlen sees them, and the scale's float bits --
a path of stays gives no call, and the statements run clean under the address and undefined-behaviour sanitizers (tests/dwell_asan.c,
a program of its own)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 300)


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "dwell", "ref_dwell.npz"))


def events_of(ref, key, annotate=True):
    """the case's event table, annotated as scrappie_events.c:308-311 annotates it"""
    ev = np.zeros(len(ref[key + "__path"]), dtype=synth.EVENT_DTYPE)
    ev["start"], ev["length"] = ref[key + "__start"], ref[key + "__length"]
    ev["mean"], ev["stdv"] = 80.0, 1.0
    ev["pos"], ev["state"] = (ref[key + "__pos"], ref[key + "__path"] + 1) if annotate else (-1, -1)
    return ev


def test_fixture_holds_every_case(ref):
    """the hand-made cases and every random length are there for both state counts, no path is all stays, and the correction changes
    at least half of the random calls (the generator asserts it; a fixture of unchanged calls would test nothing)"""
    have = [str(k) for k in ref["cases"]]
    for k in ("first_homo", "ends_inside", "ends_inside_zero", "first_homo_stays", "broken_by_stays", "two_in_succession", "leading_stays",
              "one_kmer", "no_step", "half_even", "half_odd", "half_scales", "half_scales_odd", "over_long"):
        assert k in have and int(ref["nstate_" + k]) == 1025, k
    for nstate, seeds in ((1025, 10), (65, 2)):
        for n in LENGTHS:
            for seed in range(seeds):
                k = "rand%d_%d_%d" % (nstate, n, seed)
                assert k in have and len(ref[k + "__path"]) == n and int(ref["nstate_" + k]) == nstate
    rand = [k for k in have if k.startswith("rand")]
    assert all(np.any(ref[k + "__path"] >= 0) for k in have)
    assert 2 * sum(str(ref[k + "__corrected"]) != str(ref[k + "__plain"]) for k in rand) >= len(rand)
    assert sum(int(ref["nstate_" + k]) == 1025 for k in have) > 128          # three waves of the device's kernel, the last one partial
    # the quirk of the last homopolymer, and the read that outgrows a plain call's reservation
    assert str(ref["ends_inside__dco"][0]) == "ACGTAAAAAAA" and str(ref["ends_inside_zero__dco"][0]) == "ACGTAAAAA"
    assert str(ref["first_homo__dco"][0]) == "AAAAAAAC"
    n = len(ref["over_long__path"])
    assert (5 * n + 16 + 15) // 16 * 16 < len(str(ref["over_long__corrected"])) < sa.dwell_capacity(n)


def test_fixture_provenance():
    """tests/golden/dwell/PROVENANCE.json (written by make_dwell_golden.py, in the format of events/PROVENANCE.json): the fixture is the
    file the record was made with, every fixture of the folder has a record, and -- wherever the reference checkout is present -- every
    reference file it derives from is still the file it was derived from"""
    sys.path.insert(0, GOLDEN)
    import provenance
    rec = json.load(open(os.path.join(GOLDEN, "dwell", "PROVENANCE.json")))
    seen = set()
    for pat, d in rec.items():
        assert d["fixtures"] and d["reference_files"], pat
        for f, h in d["fixtures"].items():
            assert hashlib.sha256(provenance.fixture_bytes(os.path.join(GOLDEN, f))).hexdigest() == h, f
            seen.add(f)
    assert {os.path.relpath(f, GOLDEN) for f in provenance.fixture_files("dwell/*.npz")} <= seen
    ref_dir = "/root/reference"
    if os.path.isdir(os.path.join(ref_dir, "src")):
        for pat, d in rec.items():
            for f, h in d["reference_files"].items():
                assert hashlib.sha256(open(os.path.join(ref_dir, f), "rb").read()).hexdigest() == h, f


def test_host_statements_equal_reference(ref):
    """every case: overlapper (string and pos), dwell_corrected_overlapper at the fixture's scales, homopolymer_dwell_correction, and the
    scale it divides by, bit for bit"""
    ip = sa.C.POINTER(sa.C.c_int)
    for key in (str(k) for k in ref["cases"]):
        path, nstate = ref[key + "__path"], int(ref["nstate_" + key])
        pos = np.zeros(len(path), np.int32)
        plain = sa._take_string(sa.lib().overlapper(np.ascontiguousarray(path).ctypes.data_as(ip), len(path), nstate - 1, pos.ctypes.data_as(ip)))
        assert plain == str(ref[key + "__plain"]) and np.array_equal(pos, ref[key + "__pos"]), key
        dwell = ref[key + "__length"].astype(np.int32)
        for scale, want in zip(ref[key + "__scales"], ref[key + "__dco"]):
            assert sa.dwell_corrected_overlapper(path, dwell, nstate - 1, float(scale)) == str(want), (key, scale)
        ev = events_of(ref, key)
        assert sa.homopolymer_dwell_correction(ev, path, nstate, len(plain)) == str(ref[key + "__corrected"]), key
        scale = sa.dwell_scale(ev, len(plain))
        assert np.array(scale, np.float32).view(np.uint32) == ref[key + "__scale_bits"], key
        # the scale through dwell_corrected_overlapper is the correction
        assert sa.dwell_corrected_overlapper(path, dwell, nstate - 1, float(scale)) == str(ref[key + "__corrected"]), key


def test_rounds_half_away_from_zero(ref):
    """10 / 4 = 2.5 gives three bases and 14 / 4 = 3.5 four: roundf, not the round-to-even of rintf; and the fixture's two cases whose
    dwell over homo_scale is an exact half in float, x even and x odd"""
    assert str(ref["half_scales__dco"][0]) == "ACGT" + 8 * "A" + "C" and str(ref["half_scales_odd__dco"][0]) == "ACGT" + 9 * "A" + "C"
    seen = set()
    for key in ("half_even", "half_odd"):
        scale = ref[key + "__scale_bits"].view(np.float32)
        hd = np.float32(ref[key + "__length"].astype(np.int32)[4:7].sum())
        q = np.float32(hd / scale)
        assert q % 1 == 0.5
        seen.add(int(q) % 2)
        nhomo = str(ref[key + "__corrected"]).count("A") - str(ref[key + "__plain"]).count("A")
        assert nhomo == int(q), key          # (the plain call has one A for the repeat of AAAAA, the corrected one x + 1 for the run)
    assert seen == {0, 1}


def test_no_kmer_no_call():
    """a path of stays: NULL / None from both statements, without a crash (the reference is undefined there)"""
    for n in (1, 2, 8, 9, 64):
        path = np.full(n, -1, np.int32)
        ev = np.zeros(n, dtype=synth.EVENT_DTYPE)
        ev["length"], ev["start"], ev["pos"], ev["state"] = 5.0, np.arange(n) * 5, 0, 0
        assert sa.homopolymer_dwell_correction(ev, path, 1025, 5) is None
        assert sa.dwell_corrected_overlapper(path, np.full(n, 5, np.int32), 1024, 9.0) is None
    # a scale of zero has no count to round to
    assert sa.dwell_corrected_overlapper([0, 0], [3, 7], 1024, 0.0) is None


def test_host_statements_under_sanitizers(tmp_path, ref):
    """tests/dwell_asan.c (its own main) runs the statements built with -fsanitize=address,undefined over the fixture's cases on
    buffers of exactly their length, over paths of stays, a scale of zero and a dwell of a million: no report, the fixture's strings"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "dwell_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "dwell_asan.c"), os.path.join(csrc, "sh_host.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    keys = [str(k) for k in ref["cases"] if len(ref[str(k) + "__path"]) <= 65]
    words = [np.array([len(keys)], np.int32)]
    for k in keys:
        words += [np.array([int(ref["nstate_" + k]), len(ref[k + "__path"])], np.int32), ref[k + "__path"].astype(np.int32),
                  ref[k + "__length"].astype(np.int32)]
    data = str(tmp_path / "cases.i32")
    np.concatenate(words).astype("<i4").tofile(data)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.split("\n")
    for i, k in enumerate(keys):
        assert lines[2 * i] == str(ref[k + "__corrected"]), k
        if 9.0 in ref[k + "__scales"]:
            assert lines[2 * i + 1] == str(ref[k + "__dco"][list(ref[k + "__scales"]).index(9.0)]), k
    tail = lines[2 * len(keys):]
    assert tail[:18] == ["NULL"] * 18 and tail[18] == "NULL" and int(tail[19]) == 5 + 1 + 8000000 - 1
