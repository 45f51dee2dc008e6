"""Every single-base edit of a sequence scored against a read of a transducer model (k_map_edits_rows, k_map_edits,
csrc/sh_map_edits.h), the part that needs no GPU.  np_map_edits is the definition (include/scrappie_hip.h states it in words):
np_map's forward cells kept for every entry, backward rows, and per edit its own middle columns joined to the suffix where a path
reaches it for the first time.  It is held here against np_map (pinned to the compiled reference in tests/test_map_cpu.py) on the
edited sequence (sa.apply_edit) -- in float64 to 1e-9, where the only difference is the order of additions; in float32 within the
project's standing bound for re-associated sums.  Further: the layout of a launch on the host (scrappie_hip_map_edits_plan; under
sanitizers through tests/map_edits_asan.c), the Python argument checks, the exports and the CLI's refusals."""
import os
import subprocess

import numpy as np
import pytest

import scrappie_amd as sa
from test_map_cpu import BIG, CLI, _lse, np_map
from test_map_multi_cpu import _NoEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scrappie_hip_map_edits_batch", "map_post_edits", "scrappie_hip_map_edits_pitch", "scrappie_hip_map_edits_row_bytes",
               "scrappie_hip_map_edits_plan", "scrappie_hip_map_edits_max_bases", "scrappie_hip_map_edits_form_counts",
               "scrappie_hip_map_edits_timing")
PENS = ((0.0, 0.0, 4.0), (0.3, 0.7, 2.0))
KMAX = 5                    # middle columns an edit can have: the longest k-mer of the shipped models


def encode(seq, k):
    """state codes of the k-mers of base codes `seq`, the first base the most significant (encode_bases_to_integers)"""
    seq = np.asarray(seq, dtype=np.int64)
    n = len(seq) - k + 1
    out = np.zeros(max(n, 0), dtype=np.int64)
    for j in range(k):
        out = out * 4 + seq[j:j + n]
    return out


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def np_map_edits(post, seq, k, pens, viterbi=True, dtype=np.float32):
    """(base, sub (L, 4), dele (L,), ins (L + 1, 4)) in `dtype` for post (NB, 4^k + 1) log-posteriors, stay last, and base codes
    `seq`; NaN where the edited sequence has no admissible path or fewer than k bases.  base is np_map's score as it is.
    mx(a, b): b if b > a else a (Viterbi), _lse(a, b) (forward), the arguments in the order of the definition.  The rows are
    vectorised over the cells of an entry, the edits of a kind and a new base over the positions."""
    f = np.dtype(dtype).type
    post = np.ascontiguousarray(post).astype(dtype)
    seq = np.asarray(seq, dtype=np.int64)
    NB, nr = post.shape
    L = len(seq)
    assert nr == 4 ** k + 1 and NB >= 1 and 1 <= k <= KMAX
    sub = np.full((L, 4), np.nan, dtype=dtype)
    dele = np.full(L, np.nan, dtype=dtype)
    ins = np.full((L + 1, 4), np.nan, dtype=dtype)
    if L < k:
        return f(np.nan), sub, dele, ins
    n = L - k + 1
    s = encode(seq, k)
    STAY = nr - 1
    sp, kp, lpen = f(pens[0]), f(pens[1]), f(pens[2])
    big = f(BIG)

    def mx(a, b):
        return np.where(b > a, b, a) if viterbi else _lse(a, b)

    with np.errstate(over="ignore", invalid="ignore"):
        lps_all = post[:, STAY]
        ls_all = mx(np.full(NB, -lpen, dtype=dtype), lps_all)
        # forward rows: np_map's cells, kept
        F = np.full((NB + 1, n), -big, dtype=dtype)
        FS = np.zeros(NB + 1, dtype=dtype)
        E = -big
        for t in range(NB):
            p, row, lps = F[t], post[t], lps_all[t]
            le = row[s]
            v = (p - sp) + lps
            if n > 1:
                v[1:] = mx(v[1:], p[:n - 1] + le[1:])
            if n > 2:
                v[2:] = mx(v[2:], (p[:n - 2] - kp) + le[2:])
            v[0] = mx(v[0], FS[t] + le[0])
            F[t + 1] = v
            FS[t + 1] = FS[t] + ls_all[t]
            E = mx(E + ls_all[t], p[n - 1] - lpen)
        base = (np.fmax if viterbi else _lse)(F[NB, n - 1], E)
        # backward rows
        G = np.full((NB + 1, n), -big, dtype=dtype)
        G[NB, n - 1] = 0
        GE = np.zeros(NB + 1, dtype=dtype)
        for t in range(NB - 1, -1, -1):
            row, lps, g = post[t], lps_all[t], G[t + 1]
            GE[t] = GE[t + 1] + ls_all[t]
            le = row[s]
            v = (lps - sp) + g
            if n > 1:
                v[:n - 1] = mx(v[:n - 1], le[1:] + g[1:])
            if n > 2:
                v[:n - 2] = mx(v[:n - 2], (le[2:] - kp) + g[2:])
            v[n - 1] = mx(v[n - 1], -lpen + GE[t + 1])
            G[t] = v

        def edits(kind, c):
            """the scores of the edits of this kind and new base at every position at once"""
            I = np.arange(L + 1 if kind == "ins" else L)
            if kind == "sub":
                n2, j0, A = n, np.minimum(I + 1, n), np.clip(I - k + 1, 0, n)
            elif kind == "del":
                n2, j0, A = n - 1, np.minimum(I + 1, n), np.clip(I - k + 1, 0, max(n - 1, 0))
            else:
                n2, j0, A = n + 1, np.minimum(I, n), np.clip(I - k + 1, 0, n)
            Bn = n - j0
            A = np.minimum(A, n2 - Bn)
            J = n2 - Bn
            M = J - A
            assert np.all(M >= 0) and np.all(M <= k) and np.all(A >= 0)

            def base_at(p):                                 # the edited sequence's base at p (clamped where it has none)
                cl = lambda q: seq[np.clip(q, 0, L - 1)]
                if kind == "sub":
                    return np.where(p == I, c, cl(p))
                if kind == "del":
                    return cl(np.where(p < I, p, p + 1))
                return np.where(p < I, cl(p), np.where(p == I, c, cl(p - 1)))

            mid = []
            for m in range(KMAX):
                code = np.zeros(len(I), dtype=np.int64)
                for j in range(k):
                    code = code * 4 + base_at(A + m + j)
                mid.append(code)
            s0, s1 = s[np.minimum(j0, n - 1)], s[np.minimum(j0 + 1, n - 1)]
            X = [np.full(len(I), -big, dtype=dtype) for _ in range(KMAX)]
            acc = np.full(len(I), -big, dtype=dtype)

            def ext_of(t):
                """columns A - 2, A - 1 of the prefix and the middle columns, at entry t"""
                fa1 = np.where(A >= 1, F[t][np.maximum(A - 1, 0)], -big).astype(dtype)
                fa2 = np.where(A >= 2, F[t][np.maximum(A - 2, 0)], -big).astype(dtype)
                return [fa2, fa1] + X

            def pick(ext, at):
                out = ext[0].copy()
                for j in range(1, len(ext)):
                    out = np.where(at == j, ext[j], out)
                return out

            for t in range(NB):
                row, lps, ls = post[t], lps_all[t], ls_all[t]
                ext = ext_of(t)
                c1, c2 = pick(ext, M + 1), pick(ext, M)     # columns J - 1 and J - 2 at entry t
                le0, le1 = row[s0], row[s1]
                g0, g1 = G[t + 1][np.minimum(j0, n - 1)], G[t + 1][np.minimum(j0 + 1, n - 1)]
                # no suffix: END's chain
                e = mx(acc + ls, c1 - lpen)
                # a suffix: the first arrival in it
                y0 = np.where(J == 0, FS[t], c1) + le0
                y0 = np.where(J >= 2, mx(y0, (c2 - kp) + le0), y0)
                b = mx(acc, y0 + g0)
                b = np.where((Bn >= 2) & (J >= 1), mx(b, ((c1 - kp) + le1) + g1), b)
                acc = np.where(Bn == 0, e, b).astype(dtype)
                for m in range(KMAX - 1, -1, -1):           # in place, m descending: the left neighbours are still entry t's
                    q = A + m
                    le = row[mid[m] % (nr - 1)]
                    v = (X[m] - sp) + lps
                    v = np.where(q >= 1, mx(v, ext[m + 1] + le), v)
                    v = np.where(q >= 2, mx(v, (ext[m] - kp) + le), v)
                    v = np.where(q == 0, mx(v, FS[t] + le), v)
                    X[m] = np.where(m < M, v, X[m]).astype(dtype)
            last = pick(ext_of(NB), M + 1)
            closed = np.fmax(last, acc) if viterbi else _lse(last, acc)
            out = np.where(Bn == 0, closed, acc).astype(dtype)
            out[out < -big / 2] = np.nan
            if n2 < 1:
                out[:] = np.nan
            return out

        for c in range(4):
            sub[:, c] = edits("sub", c)
            ins[:, c] = edits("ins", c)
        dele[:] = edits("del", None)
    return f(base), sub, dele, ins


def all_edits(L):
    """(kind, i, c) of every single-base edit of a sequence of L bases, in the order of pick()"""
    return ([("sub", i, c) for i in range(L) for c in range(4)] + [("del", i, None) for i in range(L)] +
            [("ins", i, c) for i in range(L + 1) for c in range(4)])


def pick(res, kind, i, c):
    base, sub, dele, ins = res
    return sub[i][c] if kind == "sub" else dele[i] if kind == "del" else ins[i][c]


def flat(res, L):
    return np.array([pick(res, *e) for e in all_edits(L)], dtype=np.float64)


def brute_edits(post, seq, k, pens, viterbi, dtype):
    """np_map on every edited sequence, as float64 values; NaN below -BIG / 2 and where fewer than k bases remain"""
    out = []
    for kind, i, c in all_edits(len(seq)):
        ed = sa.apply_edit(np.asarray(seq, dtype=np.int32), kind, i, c)
        if len(ed) < k:
            out.append(np.nan)
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            v = float(np_map(post, encode(ed, k), *pens, viterbi=viterbi, dtype=dtype)[0])
        out.append(v if v >= -float(BIG) / 2 else np.nan)
    return np.array(out, dtype=np.float64)


def make_post(nblock, k, rng, sharp=2.0, stay_low=False):
    """a log-posterior of nblock blocks over 4^k + 1 states"""
    x = rng.normal(0.0, sharp, (nblock, 4 ** k + 1))
    if stay_low:
        x[:, -1] -= 30.0                                    # the stay row below -local_pen everywhere
    x -= np.log(np.exp(x).sum(axis=1, keepdims=True))
    return x.astype(np.float32)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def map_edits_cases():
    """(name, post, seq, k, pens), fixed seeds: k = 1, 2, 3; L = k, k + 1, 2 k, 12; NB = 1, 2 and more blocks than states;
    a homopolymer; a stay row below -local_pen; both penalty sets"""
    out = []
    rng = np.random.default_rng(20261020)
    for k in (1, 2, 3):
        for L in sorted({k, k + 1, 2 * k, 12}):
            for NB in (1, 2, L + 7):
                pens = PENS[(k + L + NB) % 2]
                out.append(("k%d-L%d-nb%d" % (k, L, NB), make_post(NB, k, rng), rng.integers(0, 4, L), k, pens))
        out.append(("k%d-homopolymer" % k, make_post(17, k, rng), np.full(9, 2), k, PENS[1]))
        out.append(("k%d-stay-low" % k, make_post(15, k, rng, stay_low=True), rng.integers(0, 4, 8), k, PENS[0]))
        out.append(("k%d-other-pens" % k, make_post(14, k, rng), rng.integers(0, 4, 12), k, PENS[k % 2]))
    return [(nm, p, np.asarray(s, dtype=np.int32), k, pens) for nm, p, s, k, pens in out]


CASES = map_edits_cases()


@pytest.fixture(scope="module")
def brute():
    """per case and form: np_map on every edited sequence in float64 and float32, computed once"""
    out = {}
    for name, post, seq, k, pens in CASES:
        for vit in (True, False):
            out[name, vit] = (brute_edits(post, seq, k, pens, vit, np.float64), brute_edits(post, seq, k, pens, vit, np.float32))
    return out


def same_bits(a, b, dtype):
    a, b = dtype(a), dtype(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# the definition against np_map
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("viterbi", [True, False])
def test_float64_definition_equals_np_map_of_every_edit(brute, viterbi):
    worst, finite = 0.0, 0
    for name, post, seq, k, pens in CASES:
        res = np_map_edits(post, seq, k, pens, viterbi=viterbi, dtype=np.float64)
        want = brute[name, viterbi][0]
        got = flat(res, len(seq))
        assert got.shape == want.shape == (9 * len(seq) + 4,)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, np.flatnonzero(np.isnan(got) != np.isnan(want)))
        ok = ~np.isnan(want)
        finite += int(ok.sum())
        if len(seq) == k:
            assert np.all(np.isnan(res[2])), name                                   # every deletion leaves fewer than k bases
        err = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
        if err.size:
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-9, (name, float(err.max()))
        w = np_map(post, encode(seq, k), *pens, viterbi=viterbi, dtype=np.float64)[0]
        assert same_bits(res[0], w, np.float64), name
    assert finite > 1000
    print("float64, %s: %d finite edits, worst relative difference to np_map of the edited sequence %.3g"
          % ("viterbi" if viterbi else "forward", finite, worst))


@pytest.mark.parametrize("viterbi", [True, False])
def test_float32_definition_within_the_standing_bound(brute, viterbi):
    """|edits32 - f64| <= 2 |np_map32(edited) - f64| + 1e-5 |f64|, base in bits"""
    worst, where = 0.0, None
    for name, post, seq, k, pens in CASES:
        res = np_map_edits(post, seq, k, pens, viterbi=viterbi, dtype=np.float32)
        assert all(a.dtype == np.float32 for a in res[1:])
        f64, f32 = brute[name, viterbi]
        got = flat(res, len(seq))
        assert np.array_equal(np.isnan(got), np.isnan(f64)), name
        ok = ~np.isnan(f64)
        lhs = np.abs(got[ok] - f64[ok])
        rhs = 2 * np.abs(f32[ok] - f64[ok]) + 1e-5 * np.abs(f64[ok])
        ratio = lhs / np.where(rhs > 0, rhs, 1.0)
        if ratio.size and ratio.max() > worst:
            worst, where = float(ratio.max()), name
        assert np.all(lhs <= rhs), (name, float(np.max(lhs - rhs)))
        w = np_map(post, encode(seq, k), *pens, viterbi=viterbi, dtype=np.float32)[0]
        assert same_bits(res[0], w, np.float32), name
    print("float32, %s: worst ratio of |edits32 - f64| to its bound %.3f (%s)" % ("viterbi" if viterbi else "forward", worst, where))


def test_fewer_than_k_bases_is_nan():
    rng = np.random.default_rng(5)
    base, sub, dele, ins = np_map_edits(make_post(6, 3, rng), [0, 1], 3, PENS[0])
    assert np.isnan(base) and np.all(np.isnan(sub)) and np.all(np.isnan(dele)) and np.all(np.isnan(ins))
    assert sub.shape == (2, 4) and dele.shape == (2,) and ins.shape == (3, 4)


# ---------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------
def check_edits_plan(lens, nbs, k):
    """what the kernels rely on: a row holds the n cells and slot n, 16-byte starts, no two reads overlap, F and G apart"""
    pitch, rows, res, nrow, nres = sa.map_edits_plan(lens, nbs, k)
    spans, rspans = [], []
    for j, (L, nb) in enumerate(zip(lens, nbs)):
        n = L - k + 1
        assert pitch[j] >= n + 1 and pitch[j] % 16 == 0 and pitch[j] < n + 1 + 16 and pitch[j] == sa.lib().scrappie_hip_map_edits_pitch(L, k)
        assert rows[j] % 4 == 0 and res[j] % 4 == 0
        size = 2 * (nb + 1) * int(pitch[j])
        assert size * 4 == sa.lib().scrappie_hip_map_edits_row_bytes(L, k, nb)
        spans.append((int(rows[j]), int(rows[j]) + size))
        rspans.append((int(res[j]), int(res[j]) + 9 * L + 4))
    for sp, total in ((spans, nrow), (rspans, nres)):
        for (a0, a1), (b0, b1) in zip(sp, sp[1:]):
            assert a1 <= b0
        assert not sp or (sp[0][0] == 0 and sp[-1][1] <= total)
    return pitch, rows, res, nrow, nres


def test_plan_keeps_reads_apart():
    rng = np.random.default_rng(3)
    for k in (1, 2, 5):
        for n in (0, 1, 2, 9, 40):
            check_edits_plan([int(x) for x in rng.integers(k, 800, n)], [int(x) for x in rng.integers(1, 900, n)], k)
    pitch, rows, res, nrow, nres = check_edits_plan([5, 19, 20, 730], [1, 5, 5, 800], 5)
    assert pitch.tolist() == [16, 16, 32, 736] and rows.tolist() == [0, 64, 64 + 192, 64 + 192 + 384]
    assert res.tolist() == [0, 52, 52 + 176, 52 + 176 + 184] and nres == 52 + 176 + 184 + 6576 and nrow == 640 + 2 * 801 * 736
    assert sa.map_edits_plan([], [], 5)[3:] == (0, 0)
    with pytest.raises(ValueError):
        sa.map_edits_plan([8, 9], [5], 5)
    with pytest.raises(ValueError):
        sa.map_edits_plan([3], [5], 5)                      # fewer bases than a k-mer: no states, no rows
    L = sa.lib()
    assert L.scrappie_hip_map_edits_max_bases(5) == L.scrappie_hip_map_lds_max_seq() + 4
    assert L.scrappie_hip_map_edits_max_bases(1) == L.scrappie_hip_map_lds_max_seq()
    assert L.scrappie_hip_map_edits_pitch(3, 5) == 0 and L.scrappie_hip_map_edits_row_bytes(3, 5, 7) == 0


def test_plan_under_sanitizers(tmp_path):
    """tests/map_edits_asan.c (its own main) with sh_host.c under -fsanitize=address,undefined: the plan on arrays of exactly n entries"""
    csrc = os.path.join(ROOT, "scrappie_amd", "csrc")
    exe = str(tmp_path / "map_edits_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=gnu11", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "map_edits_asan.c"),
                        os.path.join(csrc, "sh_host.c"), "-o", exe, "-lm"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-500:]


def test_arguments_are_refused_before_any_launch():
    sigs = [np.zeros(1000, dtype=np.float32)] * 3
    f = sa.Engine.score_edits_transducer
    with pytest.raises(ValueError, match="per signal"):
        f(_NoEngine(), sigs, ["ACGTACGT", "ACGAACGT"])                          # two sequences for three reads
    with pytest.raises(TypeError):
        sa.map_post_edits(np.zeros((10, 17), dtype=np.float32), "ACGT")
    with pytest.raises(ValueError):
        sa.map_post_edits(sa.ScrappyMatrix.from_numpy(np.zeros((4, 25), dtype=np.float32), sloika=False), "ACGT")     # 24 is no 4^k


def test_edits_symbols_are_exported_and_declared():
    L = sa.lib()
    header = open(os.path.join(ROOT, "include", "scrappie_hip.h")).read()
    for nm in NEW_SYMBOLS:
        assert hasattr(L, nm), nm
        assert nm + "(" in header, nm
    forms = sa.map_edits_form_counts()
    assert len(forms) == 12 and sum(1 for f in forms if f[0] == "rows") == 8 and sum(1 for f in forms if f[0] == "edits") == 4
    assert callable(sa.map_post_edits) and callable(sa.Engine.score_edits_transducer) and callable(sa.Engine.map_edits_timing)


def test_seqmappy_kmer_edits_without_gpu(tmp_path):
    """--help names the option; the refusals that need no device: with another mode, without --reference handled as --edits's are"""
    h = subprocess.run([CLI, "seqmappy", "--help"], capture_output=True, text=True, timeout=60)
    assert "--kmer-edits" in h.stdout + h.stderr and "--edits   " in h.stdout + h.stderr
    fa = tmp_path / "a.fa"
    fa.write_text(">a\nACGTACGTAC\n")
    for other in ("--edits", "--all-records", "--inside", "--find", "--within", "--each-record"):
        r = subprocess.run([CLI, "seqmappy", "--kmer-edits", other, str(fa), "nothing.fast5"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "" and "--kmer-edits" in r.stderr and other in r.stderr.replace("--kmer-edits", ""), (other, r.stderr)
    r = subprocess.run([CLI, "seqmappy", "--model", "rnnrf_r94", "--kmer-edits", str(fa), "nothing.fast5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == "" and "--kmer-edits" in r.stderr and "(--edits)" in r.stderr, r.stderr
    r = subprocess.run([CLI, "seqmappy", "--edits", str(fa), "nothing.fast5"], capture_output=True, text=True, timeout=60)           # as it was
    assert r.returncode != 0 and r.stdout == "" and "--edits" in r.stderr and "transducer" in r.stderr, r.stderr
