"""The two paths that every engine on a launch group's posterior or transitions shares (sh_eng_post.inc): the way out of a
failed launch, and the refusal of a read whose signal leaves the supported range -- each through every family's entry point.
Last, the two edits families behind their one driver (sh_eng_edits.inc): each keeps its own counters and timing; and the two
candidate-pack families behind theirs (sh_eng_cands.inc): each keeps its own counters, buffers and pack size."""
import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    e.load_model("rnnrf_r94", model.synthetic_model("rnnrf_r94", seed=11))
    e.load_model("rgrgr_r94", model.synthetic_model("rgrgr_r94", seed=1))
    yield e
    e.close()


def _bases(n, rng):
    return "".join(rng.choice(list("ACGT"), n))


def _families():
    """per entry point: run(engine, signals, ids) -- ids: which of the prepared sequences each read maps to, where the family
    has one per read --, the counter of its kernel's forms, the form these calls launch and how often per launch group, and
    whether a result is the family's empty one"""
    rng = np.random.default_rng(83)
    cands = [_bases(30, rng) for _ in range(3)]
    reference = _bases(300, rng)
    motifs = [_bases(12, rng) for _ in range(3)]
    seqs = [_bases(30, rng) for _ in range(64)]
    return {
        "map_to_sequence-rnnrf_r94": dict(
            run=lambda e, sigs, ids: e.map_to_sequence(sigs, [seqs[i] for i in ids], model="rnnrf_r94", viterbi=True, path=True),
            counts=sa.map_crf_form_counts, form=(True, True, False), per_group=1,
            empty=lambda r: np.isnan(r[0]) and r[1] is None),
        "map_to_sequences-rgrgr_r94": dict(
            run=lambda e, sigs, ids: e.map_to_sequences(sigs, cands, model="rgrgr_r94", viterbi=True, path=True),
            counts=sa.map_pack_form_counts, form=(True, True), per_group=1,
            empty=lambda r: len(r[0]) == 3 and np.all(np.isnan(r[0])) and r[1] == -1 and r[2] is None),
        "map_to_sequences_crf-rnnrf_r94": dict(
            run=lambda e, sigs, ids: e.map_to_sequences_crf(sigs, cands, model="rnnrf_r94", viterbi=True, path=True),
            counts=sa.map_crf_pack_form_counts, form=(True, True), per_group=1,
            empty=lambda r: len(r[0]) == 3 and np.all(np.isnan(r[0])) and r[1] == -1 and r[2] is None),
        "map_to_reference-rnnrf_r94": dict(
            run=lambda e, sigs, ids: e.map_to_reference(sigs, reference, model="rnnrf_r94", viterbi=True, path=True),
            counts=sa.map_crf_local_form_counts, form=(True, True, False), per_group=2,         # both passes
            empty=lambda r: np.isnan(r[0]) and r[1:] == (None, None, None)),
        "find_sequences-rnnrf_r94": dict(
            run=lambda e, sigs, ids: e.find_sequences(sigs, motifs, model="rnnrf_r94", positions=True),
            counts=sa.crf_find_form_counts, form=(True, True), per_group=1,
            empty=lambda r: len(r[0]) == 3 and np.all(np.isnan(r[0])) and r[2] == -1),
        "map_to_sequence-rgrgr_r94": dict(
            run=lambda e, sigs, ids: e.map_to_sequence(sigs, [seqs[i] for i in ids], model="rgrgr_r94", viterbi=True, path=True),
            counts=lambda: sa.launch_form_counts()["map"], form=(True, False, True, False), per_group=1,
            empty=lambda r: np.isnan(r[0]) and r[1] is None),
    }


FAMILIES = _families()
FAILED_LAUNCH = ["map_to_sequence-rnnrf_r94", "map_to_sequences-rgrgr_r94", "map_to_sequences_crf-rnnrf_r94", "map_to_reference-rnnrf_r94",
                 "find_sequences-rnnrf_r94"]


def _same(a, b, where=()):
    """bit for bit: floats by their float32 bytes (NaN equals NaN), arrays by dtype, shape and bytes"""
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, where + (k,))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, (float, np.floating)):
        assert isinstance(b, (float, np.floating)) and np.float32(a).tobytes() == np.float32(b).tobytes(), (where, a, b)
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


@pytest.fixture(scope="module")
def forty_reads():
    rng = np.random.default_rng(61)
    return [synth.medmad_normalise(synth.synthetic_signal(int(k), 500 + i)) for i, k in enumerate(rng.integers(600, 1000, 40))]


@pytest.mark.parametrize("name", FAILED_LAUNCH)
def test_failed_launch_group(eng, forty_reads, name):
    """the second of three launch groups refused (debug option fail_run: on the host, before anything is uploaded): the call
    fails with that text and hands nothing back, the third group never runs, and the engine then gives what it gave before --
    test_gpu_map.py::test_engine_failed_launch_group for the other four entry points"""
    fam = FAMILIES[name]
    count = lambda: fam["counts"]()[fam["form"]]
    g = fam["per_group"]
    eng.set_max_launch_reads(16)
    try:
        before = count()
        first = fam["run"](eng, forty_reads, range(40))
        assert len(first) == 40 and not any(fam["empty"](r) for r in first)
        assert count() - before == 3 * g
        eng.debug_option("fail_run", 2)
        got = None
        with pytest.raises(RuntimeError, match="injected failure"):
            got = fam["run"](eng, forty_reads, range(40))
        assert got is None
        assert count() - before == 4 * g           # the first group ran, the second was refused, no third
        eng.debug_option("fail_run", 0)
        _same(fam["run"](eng, forty_reads, range(40)), first)
    finally:
        eng.debug_option("fail_run", 0)
        eng.set_max_launch_reads(16384)


@pytest.fixture(scope="module")
def good_and_huge():
    good = [synth.medmad_normalise(synth.synthetic_signal(1200 + 37 * i, 900 + i)) for i in range(5)]
    huge = (synth.synthetic_signal(2000, 91, raw_units=True) * 1000.0).astype(np.float32)
    return good, huge


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_out_of_range_read_costs_only_itself(eng, good_and_huge, name):
    """a read whose first-layer activations leave the split products' range, among five good ones of its launch group: it comes
    back as the family's empty result and is named in the error text; its group-mates' results are those of a call without it"""
    fam = FAMILIES[name]
    good, huge = good_and_huge
    alone = fam["run"](eng, good, [0, 1, 2, 3, 4])
    assert len(alone) == 5 and not any(fam["empty"](r) for r in alone)
    mixed = fam["run"](eng, good[:2] + [huge] + good[2:], [0, 1, 63, 2, 3, 4])
    err = sa.last_error()
    assert len(mixed) == 6
    assert fam["empty"](mixed[2]), mixed[2]
    assert "read 2" in err and "outside the supported range" in err, err
    _same(mixed[:2] + mixed[3:], alone)


def test_edits_families_keep_their_own_state(eng):
    """the two families of "every single-base edit" run through one driver (sh_eng_edits.inc) and keep form counters, buffers,
    budget and timing each of its own: a flip-flop call of three launches (a budget of 1 KB: every read goes alone) and a
    transducer call of one move only their own family's counters, either's timing still reports its own last call after the
    other's, and the results do not depend on which family ran first"""
    rng = np.random.default_rng(97)
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 700 + i)) for i, n in enumerate((900, 1300, 1100))]
    seqs = [_bases(40, rng) for _ in sigs]
    row_bytes = sa.lib().scrappie_hip_crf_edits_row_bytes, sa.lib().scrappie_hip_map_edits_row_bytes
    crf_rows = sum(row_bytes[0](40, len(eng.posterior(x, "rnnrf_r94"))) for x in sigs)
    map_rows = sum(row_bytes[1](40, 5, len(eng.posterior(x, "rgrgr_r94"))) for x in sigs[:2])
    moved = lambda now, before: {k: now[k] - before[k] for k in now if now[k] != before[k]}

    def call_a():
        crf, tr = sa.crf_edits_form_counts(), sa.map_edits_form_counts()
        assert len(crf) == 12 and len(tr) == 12
        eng.debug_option("crf_edits_budget_kb", 1)
        try:
            res = eng.score_edits(sigs, seqs, viterbi=True)
        finally:
            eng.debug_option("crf_edits_budget_kb", 0)
        assert moved(sa.crf_edits_form_counts(), crf) == {("rows", True, True, False): 3, ("rows", True, True, True): 3, ("edits", True, True): 3}
        assert moved(sa.map_edits_form_counts(), tr) == {}
        return res

    def call_b():
        crf, tr = sa.crf_edits_form_counts(), sa.map_edits_form_counts()
        res = eng.score_edits_transducer(sigs[:2], seqs[:2], viterbi=False)
        assert moved(sa.map_edits_form_counts(), tr) == {("rows", False, True, False): 1, ("rows", False, True, True): 1, ("edits", False, True): 1}
        assert moved(sa.crf_edits_form_counts(), crf) == {}
        return res

    def timing():
        a, b = eng.crf_edits_timing(), eng.map_edits_timing()
        assert (a["launches"], a["row_bytes"]) == (3, crf_rows), a
        assert (b["launches"], b["row_bytes"]) == (1, map_rows), b

    first = call_a(), call_b()
    assert all(np.isfinite(r[0]) and np.any(np.isfinite(r[1])) for res in first for r in res)
    timing()                                                # read after B: A's three launches are still the flip-flop family's last call
    again_b = call_b()
    again_a = call_a()
    timing()
    _same((again_a, again_b), first)


def test_banded_edits_families_keep_their_own_state(eng):
    """the same for the banded calls, whose forms are the band layer's of the one driver (EditsForm, sh_eng_edits.inc): a call of
    either family with bands of half-width 8 around the reads' paths, the second read without a band, under a budget of 1 KB (every
    read goes alone) moves the banded counters of its own family by the two reads in bands and the unbanded ones by the read
    without -- the transducer family's at 64 positions per workgroup, none at 256 --, and no counter of the other family; either's
    timing still reports its own last call (three launches, the row bytes of two bands and one full matrix) after the other's, and
    the results do not depend on which family ran first"""
    rng = np.random.default_rng(97)
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 700 + i)) for i, n in enumerate((900, 1300, 1100))]
    seqs = [_bases(40, rng) for _ in sigs]
    crf_bands = [sa.map_crf_path_band(path, 40, 8) for sc, path in eng.map_to_sequence(sigs, seqs, model="rnnrf_r94", viterbi=True, path=True)]
    map_bands = [sa.map_path_band(path, 40 - 5 + 1, 8) for sc, path in eng.map_to_sequence(sigs, seqs, model="rgrgr_r94", viterbi=True, path=True)]
    crf_bands[1] = map_bands[1] = None
    crf_rows = sa.crf_edits_band_row_bytes(*crf_bands[0]) + sa.crf_edits_band_row_bytes(*crf_bands[2]) + \
        sa.lib().scrappie_hip_crf_edits_row_bytes(40, len(eng.posterior(sigs[1], "rnnrf_r94")))
    map_rows = sa.map_edits_band_row_bytes(*map_bands[0]) + sa.map_edits_band_row_bytes(*map_bands[2]) + \
        sa.lib().scrappie_hip_map_edits_row_bytes(40, 5, len(eng.posterior(sigs[1], "rgrgr_r94")))
    counters = dict(crf=sa.crf_edits_form_counts, crf_band=sa.crf_edits_band_form_counts, tr=sa.map_edits_form_counts, tr_band=sa.map_edits_band_form_counts)
    moved = lambda now, before: {k: now[k] - before[k] for k in now if now[k] != before[k]}

    def call(option, run, vit, expect):
        before = {k: f() for k, f in counters.items()}
        assert [len(before[k]) for k in ("crf", "crf_band", "tr", "tr_band")] == [12, 12, 12, 16]
        eng.debug_option(option, 1)
        try:
            res = run(vit)
        finally:
            eng.debug_option(option, 0)
        for k, f in counters.items():
            assert moved(f(), before[k]) == expect.get(k, {}), k
        return res

    forms = lambda vit, n, *width: {("rows", vit, True, False): n, ("rows", vit, True, True): n, ("edits", vit, True) + width: n}
    call_a = lambda: call("crf_edits_budget_kb", lambda vit: eng.score_edits(sigs, seqs, viterbi=vit, bands=crf_bands), True,
                          dict(crf_band=forms(True, 2), crf=forms(True, 1)))
    call_b = lambda: call("map_edits_budget_kb", lambda vit: eng.score_edits_transducer(sigs, seqs, viterbi=vit, bands=map_bands), False,
                          dict(tr_band=forms(False, 2, 64), tr=forms(False, 1)))

    def timing():
        a, b = eng.crf_edits_timing(), eng.map_edits_timing()
        assert (a["launches"], a["row_bytes"]) == (3, crf_rows), a
        assert (b["launches"], b["row_bytes"]) == (3, map_rows), b

    first = call_a(), call_b()
    assert all(np.isfinite(r[0]) and np.any(np.isfinite(r[1])) for res in first for r in res)
    timing()                                                # read after B: A's three launches are still the flip-flop family's last call
    again_b = call_b()
    again_a = call_a()
    timing()
    _same((again_a, again_b), first)


def test_pack_families_keep_their_own_state(eng):
    """the two families of "one read against many candidates" run through one driver (sh_eng_cands.inc) and keep form counters,
    buffers and pack size each of its own: a transducer call in packs of 64 cells (a candidate of 30 bases is 26 states and
    28 cells, so the four make two packs of one launch) moves only its own counter; a flip-flop call with every candidate through
    k_map_crf (map_crf_pack_cells 0) moves neither; the flip-flop call in packs moves only its own and gives the bits of the call
    without packs; and the results do not depend on which family ran first.  All with the second pass for the path."""
    rng = np.random.default_rng(89)
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 800 + i)) for i, n in enumerate((900, 1300, 1100))]
    cands = [_bases(30, rng) for _ in range(4)]
    moved = lambda now, before: {k: now[k] - before[k] for k in now if now[k] != before[k]}

    def call(run, option, cells, own, other, launches):
        before = own(), other()
        assert len(before[0]) == 4 and len(before[1]) == 4
        eng.debug_option(option, cells)
        try:
            res = run(sigs, cands, viterbi=True, path=True)
        finally:
            eng.debug_option(option, -1)
        assert moved(own(), before[0]) == ({(True, True): launches} if launches else {})
        assert moved(other(), before[1]) == {}
        return res

    tr, crf = sa.map_pack_form_counts, sa.map_crf_pack_form_counts
    call_a = lambda: call(eng.map_to_sequences, "map_pack_cells", 64, tr, crf, 1)
    call_b = lambda: call(eng.map_to_sequences_crf, "map_crf_pack_cells", 0, crf, tr, 0)
    call_c = lambda: call(eng.map_to_sequences_crf, "map_crf_pack_cells", -1, crf, tr, 1)
    try:
        first = call_a(), call_b(), call_c()
        _same(first[2], first[1])
        for res in first:
            assert len(res) == 3
            for scores, best, path in res:
                assert len(scores) == 4 and np.all(np.isfinite(scores)) and 0 <= best < 4 and path is not None
        again_c = call_c()
        again_b = call_b()
        again_a = call_a()
        _same((again_a, again_b, again_c), first)
    finally:
        eng.debug_option("map_pack_cells", -1)
        eng.debug_option("map_crf_pack_cells", -1)
