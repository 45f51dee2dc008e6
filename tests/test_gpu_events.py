"""Event detection on the GPU (csrc/sh_events.h): the batched Engine.detect_events, the per-read detect_events, Engine.basecall_events
and `scrappie event_table` against the reference's event tables (tests/golden/events/ref_event_detect.npz) and the host statement
(scrappie_hip_detect_events_host).  Everything is compared bit for bit: the arithmetic is the reference's, operation by operation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth
from test_events_cpu import FIELDS, ref, same_table, signals  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


def same_bytes(a, b, what=""):
    """two event tables (or None twice) with the same bytes in every field"""
    assert (a is None) == (b is None), what
    if a is not None:
        assert len(a) == len(b), what
        for f in FIELDS + ("pos", "state"):
            assert np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes(), (what, f)


def with_flat_stretches(n, seed):
    """a synthetic read with a constant stretch (windows of zero variance: the FLT_MIN clamp and its denormal quotient) and a
    stretch of small samples (running sums that round)"""
    x = synth.synthetic_signal(n, seed, raw_units=True)
    if n >= 30:
        x[n // 3:n // 3 + 14] = x[n // 3]
        x[n // 2::5] *= np.float32(1e-3)
    return x


@pytest.fixture(scope="module")
def mixed():
    """65 reads -- a full wave of the serial kernels and one lane -- of mixed lengths 200 .. 3000, two of them without events (a
    constant read, a read of 5 samples) in the middle; with the host statement's table of each"""
    rng = np.random.RandomState(3)
    reads = [with_flat_stretches(int(n), 1000 + i) for i, n in enumerate(rng.randint(200, 3001, size=65))]
    reads[31] = np.full(777, 91.25, dtype=np.float32)
    reads[32] = reads[32][:5]
    want = [sa.detect_events_host(x) for x in reads]
    assert want[31] is None and want[32] is None and sum(w is None for w in want) == 2
    return reads, want


def test_fixture_cases(eng, ref, signals):
    """every case of the fixture in one batch: the reference's tables, and the host statement's"""
    keys = list(signals)
    got = eng.detect_events([signals[k] for k in keys])
    for k, ev in zip(keys, got):
        same_table(ev, ref, k)
        same_bytes(ev, sa.detect_events_host(signals[k]), k)


def test_tile_edges_and_short_reads(eng):
    """lengths around the staged tile of the serial kernels, and 11, 12, 13 (twice the long window is 12); one batch, and each alone"""
    tile = int(sa.lib().scrappie_hip_event_tile())
    lengths = [tile - 1, tile, tile + 1, 2 * tile + 5, 11, 12, 13]
    reads = [with_flat_stretches(n, 40 + n) for n in lengths]
    want = [sa.detect_events_host(x) for x in reads]
    assert sum(w is not None for w in want) >= 4
    for n, g, w in zip(lengths, eng.detect_events(reads), want):
        same_bytes(g, w, n)
    for n, x, w in zip(lengths, reads, want):
        same_bytes(eng.detect_events([x])[0], w, (n, "alone"))


def test_mixed_batch_and_launch_groups(eng, mixed, ref):
    """the batch of 65 in one launch; the same bytes when a small sample budget cuts it into three launches or more; the rounding read
    rides along in both"""
    reads, want = mixed
    reads = reads + [ref["rounding__x"]]
    want = want + [sa.detect_events_host(ref["rounding__x"])]
    count = sa.lib().scrappie_hip_event_launch_count
    before = count()
    got = eng.detect_events(reads)
    assert count() - before == 1
    for i, (g, w) in enumerate(zip(got, want)):
        same_bytes(g, w, i)
    same_table(got[-1], ref, "rounding")
    total = sum(len(x) + 1 for x in reads)
    eng.debug_option("events_budget_samples", total // 3)
    try:
        before = count()
        cut = eng.detect_events(reads)
        assert count() - before >= 3
    finally:
        eng.debug_option("events_budget_samples", 0)
    for i, (g, w) in enumerate(zip(cut, want)):
        same_bytes(g, w, (i, "cut"))
    # a read above the budget alone is refused, the others are untouched
    eng.debug_option("events_budget_samples", 1000)
    try:
        part = eng.detect_events([reads[0][:400], reads[1][:1500], reads[2][:300]])
    finally:
        eng.debug_option("events_budget_samples", 0)
    assert part[1] is None and "more than one launch may hold" in sa.last_error()
    same_bytes(part[0], sa.detect_events_host(reads[0][:400]))
    same_bytes(part[2], sa.detect_events_host(reads[2][:300]))


def test_per_read_equals_batch(eng, mixed):
    """the reference's detect_events (the process-default engine, a batch of one) gives the batch's tables; windows of a RawTable count"""
    reads, want = mixed
    for i in (0, 7, 32, 64, 31):
        same_bytes(sa.detect_events(reads[i]), want[i], i)
    assert "no peak" in sa.last_error()             # (read 31, the constant one, came last)
    x = reads[3]
    same_bytes(sa.detect_events(sa.RawTable(x, 50, len(x) - 20)), sa.detect_events_host(x[50:len(x) - 20]), "window")
    same_bytes(eng.detect_events([sa.RawTable(x, 50, len(x) - 20)])[0], sa.detect_events_host(x[50:len(x) - 20]), "window, batch")
    # other parameters than the defaults
    kw = dict(window_length1=4, window_length2=9, threshold1=2.0, threshold2=7.5, peak_height=0.35)
    same_bytes(eng.detect_events([x], **kw)[0], sa.detect_events_host(x, **kw), "parameters")


def test_basecall_events_is_the_composition(eng, ref):
    """Engine.basecall_events on two synthetic reads == by hand from the FIXTURE's event tables: event_features -> the events model's
    posterior -> decode_transducer -> overlapper (bases and score)"""
    w = model.synthetic_model("nanonet_events", seed=17, size=96)
    eng.load_model("nanonet_events", w)
    keys = ["synth_500", "synth_5000"]
    got = eng.basecall_events([ref[k + "__x"] for k in keys], "nanonet_events")
    for k, c in zip(keys, got):
        ev = np.zeros(len(ref[k + "__start"]), dtype=synth.EVENT_DTYPE)
        for f in FIELDS:
            ev[f] = ref[k + "__" + f]
        ev["pos"] = -1
        ev["state"] = -1
        post = eng.posterior(sa.event_features(ev).ravel(), "nanonet_events")
        bases, score, _ = sa._decode_post(sa.ScrappyMatrix.from_numpy(post, sloika=False))
        assert c is not None and c["nblock"] == len(ev)
        assert c["bases"] == bases and np.float32(c["score"]) == np.float32(score), k
    assert eng.basecall_events([np.full(300, 80.0, dtype=np.float32)], "nanonet_events") == [None]


def test_cli_event_table(ref, fast5_dir, tmp_path):
    """`scrappie event_table` on the bundled fast5 files, whole (--trim 0:0 --segmentation 0:50): exactly the text formatted from the
    fixture's tables, in input order; a file without events gets the reference's warning and no output"""
    keys = [str(k) for k in ref["cases"] if str(k).startswith("read_")]
    files = [os.path.join(fast5_dir, k[len("read_"):] + ".fast5") for k in keys]
    flat = str(tmp_path / "flat.f32")
    np.full(500, 70.0, dtype="<f4").tofile(flat)
    want = ""
    for k, f in zip(keys, files):
        want += "# %s\n#event\tstart\tmean\tstdv\tdwell\n" % f
        start, mean, stdv, length = (ref[k + "__" + f] for f in ("start", "mean", "stdv", "length"))      # (read once: an npz member is unpacked at every access)
        want += "".join("%d\t%d\t%f\t%f\t%d\n" % (i, start[i], float(mean[i]), float(stdv[i]), int(length[i])) for i in range(len(start)))
    r = subprocess.run([CLI, "event_table", "--trim", "0:0", "--segmentation", "0:50", files[0], flat] + files[1:], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    assert "No events returned for " + flat in r.stderr
    out = str(tmp_path / "out.tsv")
    r = subprocess.run([CLI, "event_table", "-o", out, files[2]], capture_output=True, text=True)      # the defaults: trimmed 200:10, segmented
    assert r.returncode == 0 and r.stdout == "", r.stderr
    lines = open(out).read().split("\n")
    assert lines[0] == "# " + files[2] and lines[1].startswith("#event") and len(lines) > 100
