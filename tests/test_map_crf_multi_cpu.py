"""One read of a flip-flop (CRF) model against many candidate sequences, without a GPU: the packing of candidates on the host
(scrappie_hip_map_crf_pack_plan, csrc/sh_host.c; under sanitizers through tests/map_crf_multi_asan.c), the fixture the GPU tests
rank candidates on -- checked here against the numpy restatement in float32 and float64 and against decode_crf restated --, the
Python argument checks and the exports."""
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import synth
from test_map_crf_cpu import call_of, np_decode_crf, np_map_crf
from test_map_multi_cpu import _NoEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scrappie_hip_map_crf_multi_batch", "scrappie_hip_map_trans_multi", "scrappie_hip_map_crf_pack_plan",
               "scrappie_hip_map_crf_pack_max_cells", "scrappie_hip_map_crf_pack_form_counts")


def check_plan(lens, pack_cells):
    """the properties k_map_crf_pack relies on (a candidate of L bases takes L + 1 cells); returns (pack, cell, npack)"""
    maxc = sa.map_crf_pack_max_cells()
    lim = min(pack_cells, maxc)
    pack, cell, npack = sa.map_crf_pack_plan(lens, pack_cells)
    cur, used = -1, 0
    for k, L in enumerate(lens):
        c = L + 1
        if c > maxc:
            assert pack[k] == -1 and cell[k] == -1, k
            continue
        if pack[k] == cur:
            assert cell[k] == used and used + c <= lim, k          # contiguous and disjoint; a shared pack within pack_cells
            used += c
        else:
            assert pack[k] == cur + 1 and cell[k] == 0, k          # in input order
            assert cur < 0 or used + c > lim, k                    # closed only because the candidate would not have fitted
            cur, used = int(pack[k]), c
        assert used <= maxc
    assert npack == cur + 1
    return pack, cell, npack


def test_pack_plan_properties():
    rng = np.random.default_rng(5)
    maxc = sa.map_crf_pack_max_cells()
    for pack_cells in (1, 2, 64, 256, 257, 1024, 2048, maxc, maxc + 1, 1 << 40):
        for n in (0, 1, 2, 7, 24, 96):
            lens = [int(x) for x in rng.integers(1, 700, n)]
            if n >= 7:
                lens[3] = maxc - 1
                lens[5] = maxc
                lens[6] = 1
            check_plan(lens, pack_cells)


def test_pack_plan_edges():
    maxc = sa.map_crf_pack_max_cells()
    # two columns of 32 transitions and 5 words per cell and for the spare slot, within 64 KB: 64 + 5 (c + 1) <= 16384
    assert maxc == (65536 // 4 - 64) // 5 - 1 == 3263
    pack, cell, npack = sa.map_crf_pack_plan([maxc - 1], maxc)
    assert (pack.tolist(), cell.tolist(), npack) == ([0], [0], 1)  # exactly a full pack
    pack, cell, npack = sa.map_crf_pack_plan([maxc], maxc)         # one cell too many
    assert (pack.tolist(), cell.tolist(), npack) == ([-1], [-1], 0)
    pack, cell, npack = sa.map_crf_pack_plan([40, maxc, 40], 256)  # the candidate left to k_map_crf does not close the open pack
    assert (pack.tolist(), cell.tolist(), npack) == ([0, -1, 0], [0, -1, 41], 1)
    assert sa.map_crf_pack_plan([], 256)[2] == 0
    pack, cell, npack = sa.map_crf_pack_plan([300, 10, 300, 10, 10], 100)      # smaller than a candidate: that one alone
    assert (pack.tolist(), cell.tolist(), npack) == ([0, 1, 2, 3, 3], [0, 0, 0, 0, 11], 4)
    pack, cell, npack = sa.map_crf_pack_plan([63, 63, 62, 1], 128)     # 64 + 64 fills a pack to the cell
    assert (pack.tolist(), cell.tolist(), npack) == ([0, 0, 1, 1], [0, 64, 0, 63], 2)
    pack, cell, npack = sa.map_crf_pack_plan([1, 1, 1], 1)         # a pack of one cell holds no candidate: each alone
    assert (pack.tolist(), cell.tolist(), npack) == ([0, 1, 2], [0, 0, 0], 3)


def test_pack_plan_under_sanitizers(tmp_path):
    """tests/map_crf_multi_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the planner on arrays of
    exactly ncand entries"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "map_crf_multi_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "map_crf_multi_asan.c"),
                        os.path.join(csrc, "sh_host.c"), "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]


def ranking_fixture():
    """(trans, candidates, own_at): simulated transitions of 200 blocks and decode_crf's own call of them (index 3) among decoys:
    random and half as long, the call with one substitution, random and as long, the call, the call with one deletion, the call
    with one insertion, random of 201 bases (every entry a base: the only path), random of 3 bases, the single base C"""
    trans = synth.simulated_crf_transitions(200, 3)
    own = call_of(np_decode_crf(trans)[1])[0]
    rng = np.random.default_rng(2)
    n = len(own)
    sub = own.copy()
    sub[n // 2] = (sub[n // 2] + 1 + rng.integers(0, 3)) % 4
    dele = np.delete(own, n // 3)
    ins = np.insert(own, 2 * n // 3, (own[2 * n // 3] + 1 + rng.integers(0, 3)) % 4)

    def rand(k):
        return rng.integers(0, 4, k).astype(np.int32)
    cands = [rand(n // 2), sub, rand(n), own, dele, ins, rand(201), rand(3), np.array([1], dtype=np.int32)]
    return trans, [np.ascontiguousarray(c, dtype=np.int32) for c in cands], 3


@pytest.mark.parametrize("viterbi", [True, False])
def test_own_call_wins_on_the_restatement(viterbi):
    """what the GPU test asks of map_trans_to_sequences is what the restatement gives, in float32 and in float64"""
    trans, cands, own_at = ranking_fixture()
    assert trans.shape == (200, 25) and len(cands) == 9 and len(cands[6]) == 201
    assert not any(len(c) == len(cands[own_at]) and np.array_equal(c, cands[own_at]) for i, c in enumerate(cands) if i != own_at)
    for dt in (np.float32, np.float64):
        s = np.array([np_map_crf(trans, c, viterbi=viterbi, dtype=dt)[0] for c in cands], dtype=dt)
        assert np.all(np.isfinite(s)) and int(np.argmax(s)) == own_at and np.sum(s == s[own_at]) == 1, (dt, s)
        print("%s %s: the own call wins by %.3f" % ("viterbi" if viterbi else "forward", dt.__name__, s[own_at] - np.delete(s, own_at).max()))
        assert s[own_at] - np.delete(s, own_at).max() > 1.0          # far outside float rounding
    if viterbi:
        s32 = np.float32(np_map_crf(trans, cands[own_at])[0])
        assert s32.tobytes() == np.float32(np_decode_crf(trans)[0]).tobytes()


def test_map_to_sequences_crf_arguments():
    sigs = [np.zeros(1000, dtype=np.float32)] * 3
    f = sa.Engine.map_to_sequences_crf
    with pytest.raises(ValueError, match="viterbi"):
        f(_NoEngine(), sigs, ["ACGTACGT"], viterbi=False, path=True)
    with pytest.raises(ValueError, match="candidates"):
        f(_NoEngine(), sigs, ["ACGTACGT", ["ACGTACGT"], "ACGTACGT"])           # ragged: strings and lists mixed
    with pytest.raises(ValueError, match="per signal"):
        f(_NoEngine(), sigs, [["ACGTACGT"], ["ACGTACGT", "ACGTTTTT"]])         # ragged: two lists for three reads
    with pytest.raises(TypeError):
        sa.map_trans_to_sequences(np.zeros((10, 25), dtype=np.float32), ["ACGT"])
    with pytest.raises(ValueError):
        sa.map_trans_to_sequences(sa.ScrappyMatrix.from_numpy(np.zeros((4, 5), dtype=np.float32), sloika=False), ["ACGT"])


def test_pack_symbols_are_exported():
    L = sa.lib()
    for nm in NEW_SYMBOLS:
        assert hasattr(L, nm), nm
    assert sorted(sa.map_crf_pack_form_counts()) == [(v, t) for v in (False, True) for t in (False, True)]
    assert callable(sa.set_map_crf_pack_cells) and callable(sa.Engine.map_to_sequences_crf)
