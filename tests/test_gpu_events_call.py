"""Events basecalling end to end on the GPU: the dwell correction of homopolymer lengths on the device (csrc/sh_dwell.h) against the
reference's strings (tests/golden/dwell/ref_dwell.npz) and the host statement, Engine.basecall_events(dwell=True) against the
composition of its stages, and `scrappie events`.  Everything is compared for equality: the correction is integer work and a handful
of exactly rounded float operations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    """the fixture's cases of 1025 states (the device's k-mer length), each member read once: name -> dict"""
    ref = np.load(os.path.join(GOLDEN, "dwell", "ref_dwell.npz"))
    out = {}
    for k in (str(k) for k in ref["cases"]):
        if int(ref["nstate_" + k]) != 1025:
            continue
        start, length = ref[k + "__start"], ref[k + "__length"]
        out[k] = dict(path=ref[k + "__path"], dwell=length.astype(np.int32), pos=ref[k + "__pos"], corrected=str(ref[k + "__corrected"]),
                      plain=str(ref[k + "__plain"]),
                      # decode.c:689-692: the last event's length + (float)(the span of the starts), a float addition
                      num=np.float32(length[-1]) + np.float32(int(start[-1]) - int(start[0])))
    return out


cycle_model = model.homopolymer_cycle_model      # calls with homopolymers in them: seeded synthetic weights decode to one k-mer and stays


def compose(eng, x, name="nanonet_events", **params):
    """a read's call by hand, stage by stage: (plain bases, score, dwell-corrected bases, events); None where the read has no events"""
    ev = eng.detect_events([x])[0]
    if ev is None:
        return None
    post = eng.posterior(sa.event_features(ev).ravel(), name, **{k: v for k, v in params.items() if k in ("min_prob", "tempW", "tempb")})
    pm = sa.ScrappyMatrix.from_numpy(post, sloika=False)
    nblock, nstate = post.shape
    assert nblock == len(ev)
    path = np.zeros(nblock + 1, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    score = sa.lib().decode_transducer(pm.data(), params.get("stay_pen", 0.0), params.get("skip_pen", 0.0), params.get("local_pen", 2.0),
                                       path.ctypes.data_as(ip), False)
    pos = np.zeros(nblock + 1, dtype=np.int32)
    plain = sa._take_string(sa.lib().overlapper(path.ctypes.data_as(ip), nblock + 1, nstate - 1, pos.ctypes.data_as(ip)))
    if plain is None:
        return None, score, None, len(ev)
    ann = ev.copy()
    ann["pos"], ann["state"] = pos[:nblock], path[:nblock] + 1          # scrappie_events.c:308-311
    corrected = sa.homopolymer_dwell_correction(ann, path, nstate, len(plain))
    return plain, score, corrected if corrected is not None else plain, len(ev)


@pytest.fixture(scope="module")
def reads(eng):
    """twenty synthetic pA reads of mixed lengths in no order, with the model loaded and each read's call by hand"""
    eng.load_model("nanonet_events", cycle_model())
    lens = [900, 2500, 400, 5000, 1300, 700, 3100, 250, 1800, 4200, 600, 2200, 1000, 3600, 480, 1500, 2900, 820, 5200, 1150]
    sigs = [synth.synthetic_signal(n, 7000 + i, raw_units=True) for i, n in enumerate(lens)]
    return sigs, [compose(eng, x) for x in sigs]


def test_kernel_equals_reference_in_one_launch(eng, cases):
    """k_stitch_dwell on every fixture case as ONE batch -- more than 128 reads: three waves, the last one partial -- with the capacity the
    engine reserves: every string, length and pos[] is the reference's, and no read is left to the host"""
    keys = sorted(cases)
    assert 128 < len(keys) < 192
    bases, lengths, pos, redo, _ = eng.debug_stitch_dwell([cases[k]["path"] for k in keys], [cases[k]["dwell"] for k in keys],
                                                          [cases[k]["num"] for k in keys])
    for i, k in enumerate(keys):
        assert redo[i] == 0, k
        assert bases[i] == cases[k]["corrected"] and lengths[i] == len(cases[k]["corrected"]), k
        assert np.array_equal(pos[i], cases[k]["pos"]), k
    assert sum(cases[k]["corrected"] != cases[k]["plain"] for k in keys) > len(keys) // 3


def test_trailing_entry_as_the_engine_runs_it(eng, cases):
    """the engine's form: a path entry behind the last event counts for the plain length and pos[] alone; against the host statement on
    the same arrays (the fixture's paths, their last entry without an event)"""
    keys = [k for k in sorted(cases) if len(cases[k]["path"]) >= 2]
    dwells = [cases[k]["dwell"][:-1] for k in keys]
    num = [np.float32(d[-1]) + np.float32(int(d[:-1].sum())) for d in dwells]
    bases, lengths, pos, redo, _ = eng.debug_stitch_dwell([cases[k]["path"] for k in keys], dwells, num, trailing=1)
    for i, k in enumerate(keys):
        want, hpos = sa.dwell_stitch_host(cases[k]["path"], dwells[i], 1025, num[i])
        assert redo[i] == 0 and bases[i] == want and np.array_equal(pos[i], hpos), k


def test_overflow_is_flagged_and_stays_inside(eng, cases):
    """the same launch with the over-long read on a plain call's 5 (T + 1) + 16 bytes: it is flagged, the read behind it in the bases
    buffer -- and every other read -- has its string, and not a byte of the buffer outside the strings is written"""
    keys = [k for k in sorted(cases) if k != "over_long"]
    keys.insert(70, "over_long")                  # inside the second wave, a read in front of it and one behind it
    sentinel = keys[71]
    cap = [sa.dwell_capacity(len(cases[k]["path"])) for k in keys]
    n = len(cases["over_long"]["path"])
    cap[70] = 5 * n + 16
    assert len(cases["over_long"]["corrected"]) > (cap[70] + 15) // 16 * 16
    bases, lengths, pos, redo, raw = eng.debug_stitch_dwell([cases[k]["path"] for k in keys], [cases[k]["dwell"] for k in keys],
                                                            [cases[k]["num"] for k in keys], cap=cap)
    assert redo[70] == 1 and lengths[70] == 0 and bases[70] is None
    assert len(raw[70]) == 64 and bytes(raw[70]).rstrip(b"\0") == cases["over_long"]["corrected"][:len(bytes(raw[70]).rstrip(b"\0"))].encode()
    assert bases[71] == cases[sentinel]["corrected"]
    for i, k in enumerate(keys):
        if i == 70:
            continue
        assert redo[i] == 0 and bases[i] == cases[k]["corrected"], k
        assert not np.any(raw[i][(lengths[i] + 3) // 4 * 4:]), k           # (a string is stored in words of four bases)


def same_call(got, want, what):
    plain, score, corrected, nev = want
    if corrected is None:
        assert got is None, what
        return
    assert got is not None and got["nblock"] == nev, what
    assert got["bases"] == corrected and np.float32(got["score"]) == np.float32(score), what


def test_pipeline_is_the_composition(eng, reads):
    """basecall_events(dwell=True) on twenty reads in no order, cut into at least two launch groups: every read's bases and score are
    what its stages give by hand -- detect_events, event_features, the posterior, decode_transducer, overlapper, then the host statement
    on the annotated events -- so each read's dwells followed it through the length sort and the cut"""
    sigs, want = reads
    differ = sum(w is not None and w[2] is not None and w[2] != w[0] for w in want)
    assert differ >= 4, "the correction changes %d calls: a dwell array that reached the wrong read could go unseen" % differ
    eng.set_max_launch_reads(16)
    try:
        got = eng.basecall_events(sigs, "nanonet_events", dwell=True)
        off = eng.basecall_events(sigs, "nanonet_events", dwell=False)
        default = eng.basecall_events(sigs, "nanonet_events")
    finally:
        eng.set_max_launch_reads(16384)
    for i, (g, w) in enumerate(zip(got, want)):
        same_call(g, w, i)
    for i, (a, b, w) in enumerate(zip(off, default, want)):
        assert a == b, i                                          # dwell=False is today's basecall_events
        assert (a["bases"] if a else None) == w[0], i
    assert eng.basecall_events([np.full(300, 80.0, dtype=np.float32)], "nanonet_events", dwell=True) == [None]
    # pos[] when asked for is overlapper's, over every path entry
    g = eng.basecall_events(sigs[:3], "nanonet_events", dwell=True, want_pos=1)
    p = eng.basecall_events(sigs[:3], "nanonet_events", dwell=False, want_pos=1)
    for a, b in zip(g, p):
        assert np.array_equal(a["pos"], b["pos"])


def test_one_read_equals_the_read_in_the_batch(eng, reads):
    sigs, want = reads
    whole = eng.basecall_events(sigs[:6], "nanonet_events", dwell=True)
    for k in (0, 3, 5):
        assert eng.basecall_events([sigs[k]], "nanonet_events", dwell=True) == [whole[k]]
        same_call(whole[k], want[k], k)


def test_reads_that_outgrow_their_reservation_go_to_the_host(eng, reads):
    """through the engine: with 16 bytes of bases a read (debug option dwell_tight) every longer call overflows on the device, is
    flagged there, and comes back with the host statement's string"""
    sigs, want = reads
    before = int(eng.debug_fetch("n_redo", np.uint64)[0])
    eng.debug_option("dwell_tight", 1)
    try:
        got = eng.basecall_events(sigs, "nanonet_events", dwell=True)
    finally:
        eng.debug_option("dwell_tight", 0)
    for i, (g, w) in enumerate(zip(got, want)):
        same_call(g, w, i)
    # (a call of more than 16 bases cannot fit; one of exactly 16 may be flagged too: a homopolymer's bases are counted before they are stored)
    lens = [len(w[2]) for w in want if w is not None and w[2] is not None]
    nredo = int(eng.debug_fetch("n_redo", np.uint64)[0]) - before
    assert sum(n > 16 for n in lens) >= 4 and sum(n > 16 for n in lens) <= nredo <= sum(n >= 16 for n in lens)


def test_cli_events(eng, fast5_dir, tmp_path):
    """`scrappie events` on the three bundled fast5 files and a flat read: the sequences are the composition's for the same trimming, in
    input order, the FASTA header is the reference's format string field by field, --no-dwell --format sam gives the plain calls, the
    flat file gets the warning and no record, --dump is refused"""
    import json
    w = cycle_model()
    eng.load_model("nanonet_events", w)
    mf = str(tmp_path / "events.scrm")
    model.save_model(w, mf)
    names = sorted(json.load(open(os.path.join(GOLDEN, "reads", "reads.json"))))
    files = [os.path.join(fast5_dir, n + ".fast5") for n in names]
    want, uuids = [], []
    for f in files:
        x, uuid = sa.read_raw(f)
        uuids.append(uuid)
        want.append(compose(eng, sa.RawTable(x).trim().data(as_numpy=True)))
    assert all(c is not None and c[2] is not None for c in want) and sum(c[2] != c[0] for c in want) >= 2
    flat = str(tmp_path / "flat.f32")
    np.full(2000, 70.0, dtype="<f4").tofile(flat)
    r = subprocess.run([CLI, "events", "--model-file", mf, files[0], flat] + files[1:], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "No basecall returned for " + flat in r.stderr
    lines = r.stdout.split("\n")
    assert len(lines) == 2 * len(files) + 1 and lines[-1] == ""
    head = re.compile(r'^>(\S+)  \{ "filename" : "([^"]*)", "uuid" : "([^"]*)", "normalised_score" : (-?\d+\.\d{6}),  "nevent" : (\d+),  '
                      r'"sequence_length" : (\d+),  "events_per_base" : (\d+\.\d{6}) \}$')
    for i, (f, c) in enumerate(zip(files, want)):
        plain, score, corrected, nev = c
        m = head.match(lines[2 * i])
        assert m, lines[2 * i]
        assert m.group(1) == m.group(2) == os.path.basename(f) and m.group(3) == uuids[i]
        assert m.group(4) == "%f" % (-np.float32(score) / np.float32(nev)) and int(m.group(5)) == nev and int(m.group(6)) == len(corrected)
        assert m.group(7) == "%f" % (np.float32(nev) / np.float32(len(corrected)))
        assert lines[2 * i + 1] == corrected, f
    out = str(tmp_path / "out.sam")
    r = subprocess.run([CLI, "events", "--model-file", mf, "--no-dwell", "--format", "sam", "--prefix", "p_", "-o", out] + files, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert open(out).read() == "".join("p_%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*\n" % (os.path.basename(f), c[0]) for f, c in zip(files, want))
    r = subprocess.run([CLI, "events", "--model-file", mf, "--dump", str(tmp_path / "x.h5"), files[0]], capture_output=True, text=True)
    assert r.returncode != 0 and "--dump" in r.stderr and r.stdout == ""
