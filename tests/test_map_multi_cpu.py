"""One read against many candidate sequences, without a GPU: the packing of candidates on the host
(scrappie_hip_map_pack_plan, csrc/sh_host.c; under sanitizers through tests/map_multi_asan.c), the fixture the GPU tests rank
candidates on -- checked here against the numpy restatement and the compiled reference --, and the Python argument checks."""
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import synth
from test_map_cpu import call_map, np_map, ref_decode_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENS = (0.0, 0.0, 4.0)


def check_plan(lens, pack_cells):
    """the properties k_map_pack relies on; returns (pack, cell, npack)"""
    maxc = sa.map_pack_max_cells()
    lim = min(pack_cells, maxc)
    pack, cell, npack = sa.map_pack_plan(lens, pack_cells)
    cur, used = -1, 0
    for k, L in enumerate(lens):
        c = L + 2
        if c > maxc:
            assert pack[k] == -1, k
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
    maxc = sa.map_pack_max_cells()
    for pack_cells in (1, 3, 64, 256, 257, 1024, 2048, maxc, maxc + 1, 1 << 40):
        for n in (0, 1, 2, 7, 24, 96):
            lens = [int(x) for x in rng.integers(1, 700, n)]
            if n >= 7:
                lens[3] = maxc - 2
                lens[5] = maxc - 1
                lens[6] = 1
            check_plan(lens, pack_cells)


def test_pack_plan_edges():
    maxc = sa.map_pack_max_cells()
    assert maxc == 4915                                            # (3 c + c // 3 + 1) words within 64 KB
    pack, cell, npack = sa.map_pack_plan([maxc - 2], maxc)
    assert (pack.tolist(), cell.tolist(), npack) == ([0], [0], 1)  # exactly a full pack
    pack, cell, npack = sa.map_pack_plan([maxc - 1], maxc)
    assert (pack.tolist(), cell.tolist(), npack) == ([-1], [-1], 0)
    pack, cell, npack = sa.map_pack_plan([40, maxc - 1, 40], 256)  # the candidate left to k_map does not close a pack
    assert (pack.tolist(), cell.tolist(), npack) == ([0, -1, 0], [0, -1, 42], 1)
    assert sa.map_pack_plan([], 256)[2] == 0
    pack, cell, npack = sa.map_pack_plan([300, 10, 300, 10, 10], 100)      # smaller than a candidate: that one alone
    assert (pack.tolist(), cell.tolist(), npack) == ([0, 1, 2, 3, 3], [0, 0, 0, 0, 12], 4)
    pack, cell, npack = sa.map_pack_plan([62, 62, 61, 1], 128)     # 64 + 64 fills a pack to the cell
    assert (pack.tolist(), cell.tolist(), npack) == ([0, 0, 1, 1], [0, 64, 0, 63], 2)


def test_pack_plan_under_sanitizers(tmp_path):
    """tests/map_multi_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the planner on arrays of exactly
    ncand entries"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "map_multi_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "map_multi_asan.c"), os.path.join(csrc, "sh_host.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]


def winner_fixture():
    """(post, candidates, true_at): a simulated posterior (k = 3, 400 blocks), made as test_true_sequence_outscores_random makes
    its own, and its true state sequence among decoys -- the sequence with one state substituted, with one state deleted (the
    simulated states are drawn independently, so an edit of one base is an edit of one state), and random sequences of other
    lengths, shorter and longer.  The true one is neither first nor last."""
    post, tpath = synth.simulated_posterior(400, 8, klen=3)
    true = np.array([x for x in tpath if x >= 0], dtype=np.int32)
    rng = np.random.default_rng(2)
    sub = true.copy()
    at = len(true) // 2
    sub[at] = (sub[at] + 1 + rng.integers(0, 63)) % 64
    dele = np.delete(true, len(true) // 3)
    cands = [rng.integers(0, 64, len(true) // 2).astype(np.int32), sub, rng.integers(0, 64, len(true)).astype(np.int32), true, dele,
             rng.integers(0, 64, len(true) + 37).astype(np.int32), rng.integers(0, 64, 3).astype(np.int32)]
    return post, cands, 3


@pytest.mark.parametrize("viterbi", [True, False])
def test_true_candidate_wins_on_the_reference(viterbi):
    """what the GPU test asks of map_post_to_sequences is what the restatement and the compiled reference give"""
    post, cands, true_at = winner_fixture()
    assert not any(len(c) == len(cands[true_at]) and np.array_equal(c, cands[true_at]) for i, c in enumerate(cands) if i != true_at)
    s = np.array([np.float32(np_map(post, c, *PENS, viterbi=viterbi)[0]) for c in cands])
    assert np.all(np.isfinite(s)) and int(np.argmax(s)) == true_at and np.sum(s == s[true_at]) == 1, s
    R = ref_decode_lib()
    if R is not None:
        r = np.array([call_map(R, post, c, PENS, viterbi)[0] for c in cands])
        assert int(np.argmax(r)) == true_at and np.sum(r == r[true_at]) == 1, r
        if viterbi:
            assert r.tobytes() == s.tobytes()


class _NoEngine(object):
    """stands where an Engine would: the argument checks come before anything touches the engine"""
    def __getattr__(self, name):
        raise AssertionError("the argument checks reached the engine (%s)" % name)


def test_map_to_sequences_arguments():
    sigs = [np.zeros(1000, dtype=np.float32)] * 3
    f = sa.Engine.map_to_sequences
    with pytest.raises(ValueError, match="viterbi"):
        f(_NoEngine(), sigs, ["ACGTACGT"], viterbi=False, path=True)
    with pytest.raises(ValueError, match="candidates"):
        f(_NoEngine(), sigs, ["ACGTACGT", ["ACGTACGT"], "ACGTACGT"])           # ragged: strings and lists mixed
    with pytest.raises(ValueError, match="per signal"):
        f(_NoEngine(), sigs, [["ACGTACGT"], ["ACGTACGT", "ACGTTTTT"]])         # ragged: two lists for three reads
    with pytest.raises(TypeError):
        sa.map_post_to_sequences(np.zeros((10, 65), dtype=np.float32), ["ACGT"])


def test_pack_symbols_are_exported():
    L = sa.lib()
    for nm in ("scrappie_hip_map_multi_batch", "scrappie_hip_free_map_multi_results", "scrappie_hip_map_post_multi", "scrappie_hip_map_pack_plan",
               "scrappie_hip_map_pack_max_cells", "scrappie_hip_map_pack_form_counts"):
        assert hasattr(L, nm), nm
    assert sorted(sa.map_pack_form_counts()) == [(v, t) for v in (False, True) for t in (False, True)]
