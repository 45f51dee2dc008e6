"""The layer the subcommands of `scrappie` share (scrappie_amd/csrc/scrappie_cli.c), through tests/cli_common_check.c: a program of its
own, built here with -fsanitize=address,undefined from scrappie_cli.c and the host C it calls.  Every run must end without a report
of either sanitizer, the leak check at exit included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READS = os.path.join(ROOT, "tests", "golden", "reads")
FAST5 = os.path.join(ROOT, "tests", "golden", "fast5", "read_ch228_file118.fast5")
FILES = [os.path.join(READS, f) for f in sorted(os.listdir(READS)) if f.endswith(".i16")] + [FAST5]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("cli_common") / "cli_common_check")
    b = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "cli_common_check.c")] +
                       [os.path.join(csrc, f) for f in ("scrappie_cli.c", "sh_host.c", "sh_fast5.c", "sh_h5mini.c", "sh_inflate.c")] +
                       ["-o", exe, "-lm", "-ldl"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]

    def run(*args, env=None):
        e = {k: v for k, v in os.environ.items() if k != "SCRAPPIE_MODEL_DIR"}
        e.update(env or {}, ASAN_OPTIONS="detect_leaks=1")
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=e)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
        return r
    return run


# what --trim N and --trim N:M gave in every subcommand before there was one parser (strtol, strtok + atoi, atoi + strchr alike), and for
# the other strings what `scrappie raw` made of them.  None: refused, and start / end untouched
TRIM = [("200:10", (200, 10)), ("0:0", (0, 0)), ("7", (7, 7)), ("12:", (12, 0)), (":7", (0, 7)), ("a:b", (0, 0)), ("-1:3", None), ("3:-1", None),
        ("", (0, 0))]
# chunk and percentile as given; None: refused (no colon).  Their ranges are the subcommand's to check
SEG = [("100:0", (100, 0.0)), ("0:50", (0, 50.0)), ("100", None), ("100:", (100, 0.0)), (":50", (0, 50.0)), ("2:100.0", (2, 100.0))]


def test_trim_and_segmentation_grammar(check):
    got = [l.split() for l in check("trim", *[a for a, _ in TRIM]).stdout.splitlines()]
    assert len(got) == len(TRIM)
    for (arg, want), (rc, start, end) in zip(TRIM, got):
        assert (int(rc), int(start), int(end)) == ((0,) + want if want else (-1, -7, -7)), arg
    got = [l.split() for l in check("seg", *[a for a, _ in SEG]).stdout.splitlines()]
    assert len(got) == len(SEG)
    for (arg, want), (rc, chunk, pct) in zip(SEG, got):
        assert (int(rc), int(chunk), float(pct)) == ((0,) + want if want else (-1, -7, -7.0)), arg


def _reference(path, trim_start, trim_end, chunk, pct):
    """(start, end, n, window) of a prepared read: chunk > 0, the library's trim_and_segment_raw; chunk 0, the fixed trims of
    scrappie_common.c:14-20 written out; then the library's medmad_normalise_array on the window.  None where nothing is left."""
    L = sa.lib()
    rt = L.scrappie_hip_read_raw(os.fsencode(path), True)
    assert rt.raw
    n, start, end, raw = rt.n, rt.start, rt.end, rt.raw
    if chunk > 0:
        rt = L.trim_and_segment_raw(rt, trim_start, trim_end, chunk, C.c_float(pct / 100.0))      # (frees the samples if nothing is left)
        if not rt.raw:
            return None
        start, end = rt.start, rt.end
    else:
        start = start + trim_start if n - start > trim_start else n
        end = end - trim_end if end > trim_end else 0
    x = np.ctypeslib.as_array(raw, shape=(n,)).copy()
    sa._libc.free(C.cast(raw, C.c_void_p))
    if start >= end:
        return None
    win = np.ascontiguousarray(x[start:end])
    L.medmad_normalise_array(win.ctypes.data_as(C.POINTER(C.c_float)), end - start)
    return start, end, n, win


@pytest.mark.parametrize("trim_start,trim_end,chunk,pct", [(200, 10, 100, 0), (100, 20, 100, 50), (0, 0, 0, 50), (200, 10, 0, 0)])
def test_load_read_on_the_bundled_reads(check, tmp_path, trim_start, trim_end, chunk, pct):
    lines = check("load", tmp_path, trim_start, trim_end, chunk, pct, 1, *FILES).stdout.splitlines()
    assert len(lines) == len(FILES) == 4
    for i, (f, line) in enumerate(zip(FILES, lines)):
        start, end, n, win = _reference(f, trim_start, trim_end, chunk, pct)
        assert [int(v) for v in line.split()] == [start, end, n, int(f.endswith(".fast5"))], f      # (the headerless files carry no uuid)
        assert np.fromfile(str(tmp_path / ("%d.f32" % i)), np.float32).tobytes() == win.tobytes(), f
        if chunk == 0:
            assert (start, end) == (trim_start, n - trim_end)
    # without normalisation the window is the read's own samples
    check("load", tmp_path, trim_start, trim_end, chunk, pct, 0, FAST5)
    x = sa.read_raw(FAST5)[0]
    start, end = [int(v) for v in lines[3].split()[:2]]
    assert np.fromfile(str(tmp_path / "0.f32"), np.float32).tobytes() == x[start:end].tobytes()


@pytest.mark.parametrize("chunk", [100, 0])
def test_read_shorter_than_its_trims(check, tmp_path, chunk):
    """nothing is left of the read: a zeroed table, and neither its samples nor its uuid (which trim_and_segment_raw leaves to the
    caller) are still allocated when the program ends"""
    assert sa.lib().scrappie_hip_read_raw(os.fsencode(FAST5), True).uuid
    n = len(sa.read_raw(FAST5)[0])
    for trim_start, trim_end in ((n, 0), (n - 5, 5), (0, n), (10 ** 7, 10)):
        assert check("load", tmp_path, trim_start, trim_end, chunk, 0, 1, FAST5).stdout.split() == ["0", "0", "0", "0"]
        assert not os.listdir(str(tmp_path))
    assert check("load", tmp_path, 0, 0, chunk, 0, 1, str(tmp_path / "missing.fast5")).stdout.split() == ["0", "0", "0", "0"]


def test_model_path(check, tmp_path):
    msg = "scrappie: no weights for model rgrgr_r94 (weights are data, not part of this build): give --model-file or set SCRAPPIE_MODEL_DIR\n"
    r = check("model", "rgrgr_r94", "/some/file.scrm", env={"SCRAPPIE_MODEL_DIR": str(tmp_path)})
    assert (r.stdout, r.stderr) == ("/some/file.scrm\n", "")                          # the explicit file wins
    r = check("model", "rgrgr_r94", env={"SCRAPPIE_MODEL_DIR": str(tmp_path)})
    assert (r.stdout, r.stderr) == ("%s/rgrgr_r94.scrm\n" % tmp_path, "")
    r = check("model", "rgrgr_r94")
    assert (r.stdout, r.stderr) == ("NULL\n", msg)


def _first_record(text):
    """what `scrappie seqmappy` took from a FASTA file before it shared the reader: the lines of the first record, without their
    line ends, joined; None if there is no header or no sequence"""
    seq, inside = None, False
    for line in text.split("\n"):
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            if inside:
                break
            inside = True
        elif inside and line:
            seq = (seq or "") + line
    return seq


def test_read_fasta(check, tmp_path):
    text = "stray line\n>one first read\r\nACGT\r\n\r\nAC\r\n>two\n\nGGTT\nA\n>empty\n>four\tx\nT"
    fa = tmp_path / "a.fa"
    fa.write_bytes(text.encode())
    want = [("one", "ACGTAC"), ("two", "GGTTA"), ("empty", ""), ("four", "T")]

    def records(r):
        lines = r.stdout.split("\n")[:-1]
        return [l for l in lines if l.startswith("rc=")], [tuple(l.split("\t")) for l in lines if not l.startswith("rc=")]
    assert records(check("fasta", 0, fa)) == (["rc=0"], want)
    assert records(check("fasta", 0, fa, tmp_path / "missing.fa", fa)) == (["rc=0", "rc=-1", "rc=0"], want + want)
    for limit in (1, 2, 3, 5):                                                        # at most `limit` in all, over the files
        assert records(check("fasta", limit, fa, fa)) == (["rc=0", "rc=0"], (want + want)[:limit])
    assert records(check("fasta", 0, tmp_path / "missing.fa")) == (["rc=-1"], [])
    # the first record is what seqmappy used to take
    assert records(check("fasta", 1, fa))[1][0][1] == _first_record(text) == "ACGTAC"
    for f in sorted(os.listdir(READS)):
        if f.endswith(".fa"):
            got = records(check("fasta", 1, os.path.join(READS, f)))[1]
            assert len(got) == 1 and got[0][1] == _first_record(open(os.path.join(READS, f)).read()), f
