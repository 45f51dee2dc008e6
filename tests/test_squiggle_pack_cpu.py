"""One signal against many candidate squiggles, without a GPU: the packing of candidates and their END pieces on the host
(scrappie_hip_squiggle_pack_plan / _pack_layout, csrc/sh_host.c; under sanitizers through tests/squiggle_pack_asan.c), the
exported and declared symbols, and the argument checks that launch nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS0, POS1, RIGHT, HEAD = 1 << 24, 1 << 25, 1 << 26, 1 << 30


def check_plan(npos, pack_cells):
    """the properties k_squig_pack relies on; returns (pack, cell, npack)"""
    maxc = sa.squiggle_pack_max_cells()
    lim = min(pack_cells, maxc)
    pack, cell, npack = sa.squiggle_pack_plan(npos, pack_cells)
    cur, used = -1, 0
    for k, L in enumerate(npos):
        if L == 0 or L > maxc:
            assert pack[k] == -1 and cell[k] == -1, k
            continue
        if pack[k] == cur:
            assert cell[k] == used and used + L <= lim, k          # contiguous and disjoint; a shared pack within pack_cells
            used += L
        else:
            assert pack[k] == cur + 1 and cell[k] == 0, k          # input order
            assert cur < 0 or used + L > lim, k                    # closed exactly when the candidate would have passed pack_cells
            cur, used = pack[k], L
    assert npack == cur + 1
    return pack, cell, npack


def check_pieces(npos, pack, cell, which):
    """every candidate's END pieces cover exactly its cells: consecutive piece indices, one per group of 64 cells it touches, headed
    by the first of its cells there"""
    wa, wb, piece0, npiece, total = sa.squiggle_pack_layout(npos, pack, which)
    members = [k for k in range(len(npos)) if pack[k] == which]
    assert len(wa) == sum(npos[k] for k in members)
    owner = {}
    nxt = 0
    for j, k in enumerate(members):
        f, L = int(cell[k]), npos[k]
        assert piece0[k] == nxt and npiece[k] == (f + L - 1) // 64 - f // 64 + 1 <= (L + 63) // 64 + 1
        for pos in range(L):
            g = f + pos
            assert wa[g] & 0xfff == pos and (wa[g] >> 12) & 0xfff == j
            assert bool(wa[g] & POS0) == (pos == 0) and bool(wa[g] & POS1) == (pos == 1) and bool(wa[g] & RIGHT) == (pos <= L - 2)
            piece = wb[g] & 0xfff
            assert piece0[k] <= piece < piece0[k] + npiece[k]
            assert owner.setdefault(piece, (k, g // 64)) == (k, g // 64)          # a piece: one candidate, one group of 64 cells
            assert bool(wb[g] & HEAD) == (pos == 0 or g % 64 == 0)
        nxt += npiece[k]
    assert total == nxt == len(owner)
    assert all(piece0[k] == -1 and npiece[k] == -1 for k in range(len(npos)) if pack[k] != which)
    return npiece


def test_plan_order_and_closing():
    maxc = sa.squiggle_pack_max_cells()
    assert 64 <= maxc <= 0xfff
    pack, cell, n = check_plan([40] * 24, 256)
    assert n == 4 and list(pack[:7]) == [0] * 6 + [1] and list(cell[:7]) == [0, 40, 80, 120, 160, 200, 0]
    pack, cell, n = check_plan([100, 156, 1, 255, 1, 1], 256)          # exactly 256 stays open; one more closes
    assert list(pack) == [0, 0, 1, 1, 2, 2]
    pack, cell, n = check_plan([maxc, maxc + 1, 3, 0, 5], maxc)
    assert list(pack) == [0, -1, 1, -1, 1] and list(cell) == [0, -1, 0, -1, 3]
    pack, cell, n = check_plan([300, 10, 400, 10], 64)                  # pack_cells smaller than a candidate: a pack of its own
    assert list(pack) == [0, 1, 2, 3]
    pack, cell, n = sa.squiggle_pack_plan([], 256)
    assert n == 0 and len(pack) == 0
    rng = np.random.default_rng(5)
    for pc in (1, 64, 128, 256, 512, 1024, maxc):
        for _ in range(20):
            npos = [int(x) for x in rng.integers(0, 2 * maxc if rng.random() < 0.2 else 90, rng.integers(0, 30))]
            pack, cell, n = check_plan(npos, pc)
            for q in range(n):
                check_pieces(npos, pack, cell, q)


def test_end_pieces_cover_their_candidates():
    maxc = sa.squiggle_pack_max_cells()
    npos = [2, 1, 3, 257, 1, 63, 2, 64, 3, 65, 4]
    pack, cell, n = check_plan(npos, maxc)
    assert n == 1
    npiece = check_pieces(npos, pack, cell, 0)
    assert cell[3] == 6 and npiece[3] == 5              # starts mid-wave, spans four lane edges, among them the chunk edge at 256
    assert cell[5] == 264 and npiece[5] == 2            # cells 264 .. 326: over the lane edge at 320
    assert cell[7] == 329 and npiece[7] == 2
    assert list(npiece[:3]) == [1, 1, 1]
    pack, cell, n = check_plan([64, 64, 128, 1], 256)   # aligned candidates: one piece per 64 cells, none shared
    assert list(check_pieces([64, 64, 128, 1], pack, cell, 0)[:3]) == [1, 1, 2]


def test_pack_plan_under_sanitizers(tmp_path):
    """tests/squiggle_pack_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the planner and the piece tables on
    arrays of exactly the sizes they are documented to touch"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "squiggle_pack_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "squiggle_pack_asan.c"), os.path.join(csrc, "sh_host.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]


NEW = ["scrappie_hip_squiggle_match_multi_batch", "scrappie_hip_free_squiggle_multi_results", "scrappie_hip_squiggle_match_multi",
       "scrappie_hip_squiggle_pack_plan", "scrappie_hip_squiggle_pack_max_cells", "scrappie_hip_squiggle_pack_layout",
       "scrappie_hip_squiggle_pack_form_counts"]


def test_symbols_exported_and_declared():
    L = sa.lib()
    text = open(os.path.join(ROOT, "include", "scrappie_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "scrappie_hip_squiggle_candidates" in text and "scrappie_hip_squiggle_multi_result" in text
    assert sorted(sa.squiggle_pack_form_counts()) == [False, True]
    for name in ("match_squiggles", "mappy_multi"):
        assert callable(getattr(sa.Engine, name))


def test_argument_errors_without_gpu():
    """NAN and a text, and nothing is launched (this runs without a GPU)"""
    L = sa.lib()
    params, sig, _ = synth.simulated_squiggle(10, 1)
    fp = C.POINTER(C.c_float)
    rt = sa._RawTable(None, len(sig), 0, len(sig), sig.ctypes.data_as(fp))
    tg = (sa._SquigTarget * 2)(sa._SquigTarget(params.ctypes.data_as(fp), 10, 3), sa._SquigTarget(params.ctypes.data_as(fp), 10, 3))
    score = np.zeros(2, dtype=np.float32)
    sp = score.ctypes.data_as(fp)
    good = (1.0, 0.0, 2.0, 5000.0, 5.0)

    def one(rt, tg, n, pens, sp, word):
        score[:] = 0
        p = sa._SquigParams(*pens)
        assert L.scrappie_hip_squiggle_match_multi(rt, tg, n, C.byref(p), 1, sp) == -1, word
        assert word in sa.last_error(), (word, sa.last_error())

    one(rt, None, 2, good, sp, "null")
    one(rt, tg, 2, good, None, "null")
    one(rt, tg, 2, (0.0,) + good[1:], sp, "rate")
    assert np.all(np.isnan(score))
    one(rt, tg, 2, (1.0, 1.5) + good[2:], sp, "prob_back")
    one(sa._RawTable(None, len(sig), 5, 5, sig.ctypes.data_as(fp)), tg, 2, good, sp, "empty")
    one(sa._RawTable(None, len(sig), 0, len(sig) + 1, sig.ctypes.data_as(fp)), tg, 2, good, sp, "past")
    one(sa._RawTable(None, len(sig), 0, len(sig), None), tg, 2, good, sp, "signal")
    p = sa._SquigParams(*good)
    assert L.scrappie_hip_squiggle_match_multi(rt, tg, 0, C.byref(p), 1, None) == 0          # no candidates: nothing to do
    out = (sa._SquigMultiResult * 1)()
    cd = (sa._SquigCandidates * 1)()
    cd[0].cand, cd[0].ncand = tg, 2
    rts = (sa._RawTable * 1)(rt)
    assert L.scrappie_hip_squiggle_match_multi_batch(None, rts, cd, 1, C.byref(p), 1, 0, out) == -1 and "null" in sa.last_error()
    L.scrappie_hip_free_squiggle_multi_results(None, 3)
    # the Python layer
    with pytest.raises(ValueError):
        sa.Engine.match_squiggles(object(), [sig], [params], viterbi=False, path=True)
    with pytest.raises(ValueError):
        sa.Engine.match_squiggles(object(), [sig, sig], [[params]], viterbi=True)          # one list per signal
    with pytest.raises(TypeError):
        sa.squiggle_match_many(sig, [params])
    with pytest.raises(ValueError):
        sa.squiggle_match_many(sa.RawTable(sig), [params[0]])
