"""Block-based mapping (map_to_sequence_*, are_bounds_sane, encode_bases_to_integers, map_post_to_sequence,
`scrappie seqmappy`) without a GPU.

The second pin of the mapping kernels lives here: `np_map`, a numpy restatement of the four recursions of
decode.c:1420-1964 (banded quirks included), vectorised over positions.  In float32 it must equal the reference's own
compiled code (oracle/_ref/libref_decode.so) bit for bit for Viterbi, score and path; tests/test_gpu_map.py holds the
GPU against both."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import scrappie_amd as sa
from scrappie_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "scrappie_amd", "scrappie")
BIG = np.float32(1e30)


# ---------------------------------------------------------------------------
# numpy restatement of decode.c:1420-1964
# ---------------------------------------------------------------------------
def _lse(x, y):
    """util.h:162-164 in the array's own precision"""
    return np.fmax(x, y) + np.log1p(np.exp(-np.abs(x - y)))


def np_map(post, seq, stay_pen, skip_pen, local_pen, viterbi=True, low=None, high=None, dtype=np.float32):
    """(score, path or None): post (nblock, nr) log-posterior, stay last; seq state codes; bands (low, high) or None.
    The path (unbanded Viterbi only) holds positions, -1 for START and END."""
    f = np.dtype(dtype).type
    post = np.asarray(post).astype(dtype)
    seq = np.asarray(seq, dtype=np.int64)
    nblock, nr = post.shape
    L = len(seq)
    START, END, STAY = L, L + 1, nr - 1
    sp, kp, lp_ = f(stay_pen), f(skip_pen), f(local_pen)
    F = np.fmax if viterbi else _lse
    if low is None:
        c = np.full(L + 2, -f(BIG), dtype=dtype)
        c[START] = 0
        tb = np.zeros((nblock, L + 2), dtype=np.int64) if viterbi else None
        for blk in range(nblock):
            p, c = c, np.empty_like(c)
            row = post[blk]
            lps = row[STAY]
            le = row[seq]
            ls = F(-lp_, lps)
            c[START] = p[START] + ls
            e = p[END] + ls
            v = (p[:L] - sp) + lps
            if viterbi:
                src = np.arange(L)
                st = p[:max(L - 1, 0)] + le[1:]
                m = st > v[1:]
                v[1:] = np.where(m, st, v[1:]); src[1:] = np.where(m, src[1:] - 1, src[1:])
                sk = (p[:max(L - 2, 0)] - kp) + le[2:]
                m = sk > v[2:]
                v[2:] = np.where(m, sk, v[2:]); src[2:] = np.where(m, np.arange(max(L - 2, 0)), src[2:])
                fs = p[START] + le[0]
                if fs > v[0]:
                    v[0] = fs; src[0] = START
                tb[blk, :L] = src
                tb[blk, START] = START
                tb[blk, END] = END
                if p[L - 1] - lp_ > e:
                    e = p[L - 1] - lp_; tb[blk, END] = L - 1
            else:
                if L > 1:
                    v[1:] = _lse(v[1:], p[:L - 1] + le[1:])
                if L > 2:
                    v[2:] = _lse(v[2:], (p[:L - 2] - kp) + le[2:])
                v[0] = _lse(v[0], p[START] + le[0])
                e = _lse(e, p[L - 1] - lp_)
            c[:L] = v
            c[END] = e
        score = F(c[L - 1], c[END])
        if not viterbi:
            return score, None
        path = np.zeros(nblock, dtype=np.int64)
        path[-1] = L - 1 if c[L - 1] > c[END] else END
        for blk in range(nblock - 1, 0, -1):
            path[blk - 1] = tb[blk, path[blk]]
        path[path >= L] = -1
        return score, path.astype(np.int32)
    low = np.asarray(low, dtype=np.int64)
    high = np.asarray(high, dtype=np.int64)
    p = np.full(L + 2, -f(BIG), dtype=dtype)
    c = np.full(L + 2, -f(BIG), dtype=dtype)
    p[START] = 0
    row = post[0]
    lps = row[STAY]
    ls = F(-lp_, lps)
    c[START] = p[START] + ls
    c[END] = p[END] + ls
    c[0] = F(c[0], (p[0] + lps) - sp)
    if high[0] > 0:
        c[1] = row[seq[1]]
    if high[0] > 1:
        c[2] = row[seq[2]] - kp
    c[END] = F(c[END], p[START] - lp_)
    c[0] = F(c[0], p[START] + row[seq[0]])
    c[END] = F(c[END], p[L - 1] - lp_)
    for blk in range(1, nblock):
        p, c = c, p
        row = post[blk]
        lps = row[STAY]
        ls = F(-lp_, lps)
        c[START] = p[START] + ls
        c[END] = p[END] + ls
        a, b = low[blk], high[blk - 1]
        if b > a:
            c[a:b] = (p[a:b] - sp) + lps
        a, b = max(low[blk], low[blk - 1] + 1), min(high[blk], high[blk - 1] + 1)
        if b > a:
            c[a:b] = F(p[a - 1:b - 1] + row[seq[a:b]], c[a:b])
        a, b = max(low[blk], low[blk - 1] + 2), min(high[blk], high[blk - 1] + 2)
        if b > a:
            c[a:b] = F((p[a - 2:b - 2] - kp) + row[seq[a:b]], c[a:b])
        if low[blk] == 0:
            c[0] = F(c[0], p[START] + row[seq[0]])
        c[END] = F(c[END], p[L - 1] - lp_)
    return F(c[L - 1], c[END]), None


# ---------------------------------------------------------------------------
# the compiled reference
# ---------------------------------------------------------------------------
def ref_decode_lib():
    R = oracle.ref_decode()
    if R is None:
        return None
    PM, ip, sp = C.POINTER(oracle.Mat), C.POINTER(C.c_int), C.POINTER(C.c_size_t)
    R.map_to_sequence_viterbi.restype = C.c_float
    R.map_to_sequence_viterbi.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t, ip]
    R.map_to_sequence_forward.restype = C.c_float
    R.map_to_sequence_forward.argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t]
    for nm in ("map_to_sequence_viterbi_banded", "map_to_sequence_forward_banded"):
        getattr(R, nm).restype = C.c_float
        getattr(R, nm).argtypes = [PM, C.c_float, C.c_float, C.c_float, ip, C.c_size_t, sp, sp]
    R.are_bounds_sane.restype = C.c_bool
    R.are_bounds_sane.argtypes = [sp, sp, C.c_size_t, C.c_size_t]
    return R


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _sp(a):
    return a.ctypes.data_as(C.POINTER(C.c_size_t))


def call_map(L, post, seq, pens, viterbi, bands=None, cast=None):
    """one map_to_sequence_* call of library L (the reference or this build) on a numpy posterior: (score, path or None)"""
    m = oracle.NpMat(post)
    ptr = m.ptr if cast is None else C.cast(m.ptr, cast)
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    if bands is None:
        if viterbi:
            path = np.zeros(post.shape[0], dtype=np.int32)
            s = L.map_to_sequence_viterbi(ptr, *pens, _ip(seq), len(seq), _ip(path))
            return np.float32(s), path
        return np.float32(L.map_to_sequence_forward(ptr, *pens, _ip(seq), len(seq))), None
    lo, hi = (np.ascontiguousarray(b, dtype=np.uintp) for b in bands)
    fn = L.map_to_sequence_viterbi_banded if viterbi else L.map_to_sequence_forward_banded
    return np.float32(fn(ptr, *pens, _ip(seq), len(seq), _sp(lo), _sp(hi))), None


# ---------------------------------------------------------------------------
# the cases both pins are checked on
# ---------------------------------------------------------------------------
PENS = [(0.0, 0.0, 4.0), (0.5, 1.5, 2.0), (100.0, 150.0, 120.0)]


def _true_seq(path, nk, rng):
    s = [int(x) for x in path if x >= 0]
    return np.array(s if len(s) >= 3 else rng.integers(0, nk, 3), dtype=np.int32)


def map_cases(big=True):
    """(name, post, seq, pens) -- simulated posteriors for k = 3, 4, 5 and a flat one (near-ties); true, mutated and
    random sequences, lengths 1, 2, 3, ~400, ~8000 and above 2 x nblock; nblock 1, 2, 800 (and 16 000 when big)"""
    rng = np.random.default_rng(11)
    out = []
    j = 0
    for k in (3, 4, 5):
        nk = 4 ** k
        for T in (1, 2, 800):
            post, tpath = synth.simulated_posterior(T, 100 * k + T, klen=k)
            true = _true_seq(tpath, nk, rng)
            mut = true.copy()
            idx = rng.random(len(mut)) < 0.15
            mut[idx] = rng.integers(0, nk, int(idx.sum()))
            seqs = [("true", true), ("mutated", mut), ("random", rng.integers(0, nk, max(3, len(true))).astype(np.int32))]
            for n in (1, 2, 3, 400, 2 * T + 7):
                seqs.append(("len%d" % n, rng.integers(0, nk, n).astype(np.int32)))
            for name, s in seqs:
                out.append(("k%d_T%d_%s" % (k, T, name), post, s, PENS[j % 3]))
                j += 1
    flat = synth.fixture_posterior(800, 5, klen=5, hp=-1)
    for pens in PENS:
        out.append(("flat_%g" % pens[2], flat, rng.integers(0, 1024, 400).astype(np.int32), pens))
    if big:
        post, tpath = synth.simulated_posterior(16000, 77, klen=5)
        out.append(("k5_T16000_true", post, _true_seq(tpath, 1024, rng), PENS[0]))
        out.append(("k5_T16000_len8000", post, rng.integers(0, 1024, 8000).astype(np.int32), PENS[1]))
    return out


def random_bands(nblock, L, rng, mode="random"):
    """valid (low, high) bands: random monotone ones, with high[0] = 1, or with low[i] == high[i-1] where it can be"""
    high = np.sort(rng.integers(1, L + 1, nblock))
    high[-1] = L
    low = np.zeros(nblock, dtype=np.int64)
    for i in range(1, nblock):
        lo_i = int(rng.integers(low[i - 1], high[i - 1] + 1))
        if mode == "touch":
            lo_i = int(high[i - 1])
        low[i] = min(lo_i, high[i])
    if mode == "high1":
        high[0] = 1
    return low.astype(np.uintp), high.astype(np.uintp)


def band_sets(nblock, L, rng):
    """the bands a case is checked with: scrappy's diagonal (where it is valid), random, high[0] = 1, touching"""
    out = []
    if L >= 3:
        out.append(("diag", sa.diagonal_bands(3, nblock, L)))
        for mode in ("random", "high1", "touch"):
            out.append((mode, random_bands(nblock, L, rng, mode)))
    return out


def _sane(lo, hi, nblock, L):
    return sa.lib().are_bounds_sane(_sp(lo), _sp(hi), nblock, L)


# ---------------------------------------------------------------------------
# the scratch home: sequences of more than M states, whose rows live in device scratch and whose codes are read from
# global memory (sh_map.h).  map_cases reaches it with two dense unbanded reads only.
# ---------------------------------------------------------------------------
SCRATCH_NBLOCK = (1, 2, 3, 40, 41)
SCRATCH_NBLOCK_PAIRS = ((1, 2), (3, 40), (41, 2), (40, 1), (2, 3), (41, 40), (1, 40))      # one of each parity per length
SCRATCH_BAND_NBLOCK = 5600
RIDE_NBLOCK = 14000          # the simulated posterior emits a state in about 45 % of its blocks: more than M + 1 states


def lds_max_seq():
    return int(sa.lib().scrappie_hip_map_lds_max_seq())


def scratch_seqlens(M):
    """M (the last LDS size: the control), M + 1, M + 2; the next multiple of 64 and one past it; one past the next
    multiple of 256 (a chunk of the kernel's 256 threads more); about 1.5 M.  For M = 5460: 5460, 5461, 5462, 5504, 5505,
    5633, 8000."""
    r64 = (M + 3 + 63) // 64 * 64
    r256 = (r64 + 2 + 255) // 256 * 256
    return (M, M + 1, M + 2, r64, r64 + 1, r256 + 1, M * 3 // 2 // 1000 * 1000)


def map_form(post, seq, bands, viterbi, tiled=False, M=None):
    """the k_map instantiation a case runs in: (viterbi, banded, tiled, scratch) -- the key of sa.launch_form_counts()"""
    M = lds_max_seq() if M is None else M
    return (bool(viterbi), bands is not None, bool(tiled), len(seq) > M)


def _fit(seq, L, rng, nk):
    """seq cut or padded with random codes to L states"""
    seq = np.asarray(seq, dtype=np.int32)[:L]
    return np.concatenate([seq, rng.integers(0, nk, L - len(seq)).astype(np.int32)])


def map_scratch_cases():
    """(name, post, seq, pens, band sets) for k = 3 posteriors (65 states).  Unbanded (band sets None): every length of
    scratch_seqlens with two of the block counts 1, 2, 3, 40, 41 -- both ping-pong parities, the END-bit word of a short
    read -- and one read of SCRATCH_BAND_NBLOCK blocks at M + 1, whose path crosses thousands of positions.  Banded: the
    SCRATCH_BAND_NBLOCK posterior against true, mutated and random sequences of every length, with band_sets."""
    M = lds_max_seq()
    rng = np.random.default_rng(17)
    nk = 64
    out = []
    posts = {nb: synth.simulated_posterior(nb, 500 + nb, klen=3)[0] for nb in SCRATCH_NBLOCK}
    for j, L in enumerate(scratch_seqlens(M)):
        for i, nb in enumerate(SCRATCH_NBLOCK_PAIRS[j]):
            out.append(("scr_L%d_T%d" % (L, nb), posts[nb], rng.integers(0, nk, L).astype(np.int32), PENS[(2 * j + i) % 3], None))
    post, tpath = synth.simulated_posterior(SCRATCH_BAND_NBLOCK, 501, klen=3)
    true = _true_seq(tpath, nk, rng)
    mut = true.copy()
    idx = rng.random(len(mut)) < 0.15
    mut[idx] = rng.integers(0, nk, int(idx.sum()))
    kinds = [("true", true), ("mutated", mut), ("random", np.zeros(0, dtype=np.int32))]
    out.append(("scr_L%d_T%d_true" % (M + 1, SCRATCH_BAND_NBLOCK), post, _fit(true, M + 1, rng, nk), PENS[1], None))
    for j, L in enumerate(scratch_seqlens(M)):
        kind, base = kinds[j % 3]
        seq = _fit(base, L, rng, nk)
        out.append(("scr_band_L%d_%s" % (L, kind), post, seq, PENS[(j + 1) % 3], band_sets(SCRATCH_BAND_NBLOCK, L, rng)))
    # bands whose LOW edge is the true path of a posterior simulated from the sequence itself: the best path enters a
    # block through the band's lowest cell whenever it moves on, by the step whose range starts at
    # max(low[blk], low[blk - 1] + 1) -- a cell the other bands leave to worse paths.  The alignment has to beat the
    # banded forms' START -> END of block 0, so the sequence is the true one throughout and END costs 4 per block
    # (PENS[0]).  One in each home.
    for L in (M, M + 1):
        out.append(riding_case(L))
    return out


def riding_case(L, widths=(3, 40)):
    """(name, post, seq, PENS[0], [(name, (low, high))]): a k = 3 posterior simulated until its true sequence has L states,
    that sequence, and bands low[blk] = the true position at blk (0 before the first), high = low + w"""
    post, tpath = synth.simulated_posterior(RIDE_NBLOCK, 502, klen=3)
    emit = np.asarray(tpath) >= 0
    assert np.all(np.asarray(tpath) >= -1) and int(emit.sum()) > L
    nb = int(np.nonzero(np.cumsum(emit) == L)[0][0]) + 1
    post, emit = post[:nb], emit[:nb]
    seq = np.asarray(tpath)[:nb][emit].astype(np.int32)
    low = np.maximum(np.cumsum(emit) - 1, 0)
    bsets = []
    for w in widths:
        high = np.minimum(low + w, L)
        high[-1] = L
        bsets.append(("ride%d" % w, (low.astype(np.uintp), high.astype(np.uintp))))
    return ("scr_band_L%d_ride" % L, np.ascontiguousarray(post), seq, PENS[0], bsets)


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
def test_encode_bases_matches_reference():
    P = oracle.ref_pure()
    if P is None:
        pytest.skip("oracle/_ref/libref_pure.so not built")
    P.encode_bases_to_integers.restype = C.c_void_p
    P.encode_bases_to_integers.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t]
    L = sa.lib()
    rng = np.random.default_rng(3)
    for trial in range(400):
        k = 1 + trial % 5
        n = int(rng.integers(k, 60))
        s = "".join(rng.choice(list("ACGTacgt"), n))
        if trial % 7 == 0:
            s = s[:n // 2] + rng.choice(list("NnX-")) + s[n // 2 + 1:]
        b = s.encode()
        a, r = L.encode_bases_to_integers(b, len(b), k), P.encode_bases_to_integers(b, len(b), k)
        assert bool(a) == bool(r), s
        if a:
            m = len(b) - k + 1
            got = np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_int)), shape=(m,)).copy()
            want = np.ctypeslib.as_array(C.cast(r, C.POINTER(C.c_int)), shape=(m,)).copy()
            sa._libc.free(a); sa._libc.free(r)
            assert np.array_equal(got, want), s
    # n < state_len: undefined in the reference; NULL here, with a reason
    assert not L.encode_bases_to_integers(b"ACG", 3, 5)
    assert "window" in sa.last_error()


def test_are_bounds_sane_matches_reference(capfd):
    R = ref_decode_lib()
    if R is None:
        pytest.skip("oracle/_ref/libref_decode.so not built")
    rng = np.random.default_rng(5)
    nsane = 0
    for trial in range(10000):
        nb = int(rng.integers(1, 12))
        L = int(rng.integers(1, 20))
        lo, hi = random_bands(nb, L, rng, ("random", "high1", "touch")[trial % 3])
        if trial % 2:
            lo, hi = lo.copy(), hi.copy()
            i = int(rng.integers(nb))
            (lo if rng.random() < 0.5 else hi)[i] = int(rng.integers(0, L + 3))
        want = R.are_bounds_sane(_sp(lo), _sp(hi), nb, L)
        assert sa.lib().are_bounds_sane(_sp(lo), _sp(hi), nb, L) == want, (lo, hi, L)
        nsane += want
    capfd.readouterr()
    assert 2000 < nsane < 9000


@pytest.mark.parametrize("viterbi", [True, False])
def test_restatement_equals_reference(viterbi):
    """the numpy restatement against decode.c as compiled: Viterbi bit for bit (score and path), forward within float32
    rounding; full and banded"""
    R = ref_decode_lib()
    if R is None:
        pytest.skip("oracle/_ref/libref_decode.so not built")
    rng = np.random.default_rng(9)
    for name, post, seq, pens in map_cases(big=False):
        want_s, want_p = call_map(R, post, seq, pens, viterbi)
        got_s, got_p = np_map(post, seq, *pens, viterbi=viterbi)
        if viterbi:
            assert np.float32(got_s).tobytes() == want_s.tobytes(), name
            assert np.array_equal(got_p, want_p), name
        else:
            assert abs(float(got_s) - float(want_s)) <= 1e-5 * abs(float(want_s)) + 1e-4, name
        if len(seq) < 3:
            continue
        for bname, bands in band_sets(post.shape[0], len(seq), rng):
            if not _sane(bands[0], bands[1], post.shape[0], len(seq)):
                continue
            want_s, _ = call_map(R, post, seq, pens, viterbi, bands)
            got_s, _ = np_map(post, seq, *pens, viterbi=viterbi, low=bands[0], high=bands[1])
            if viterbi:
                assert np.float32(got_s).tobytes() == want_s.tobytes(), (name, bname)
            else:
                assert abs(float(got_s) - float(want_s)) <= 1e-5 * abs(float(want_s)) + 1e-4, (name, bname)


def test_scratch_cases_cover_the_scratch_home(capfd):
    R = ref_decode_lib()
    if R is None:
        pytest.skip("oracle/_ref/libref_decode.so not built")
    M = lds_max_seq()
    assert 256 < M < 65536
    if M == 5460:
        assert scratch_seqlens(M) == (5460, 5461, 5462, 5504, 5505, 5633, 8000)
    lens = scratch_seqlens(M)
    assert len(set(lens)) == 7 and lens[3] % 64 == 0 and lens[4] == lens[3] + 1 and (lens[5] - 1) % 256 == 0
    assert lens[5] > lens[4] and 1.4 * M < lens[6] < 1.6 * M
    cases = map_scratch_cases()
    assert len({c[0] for c in cases}) == len(cases)
    forms = set()
    n_sane = 0
    for name, post, seq, pens, bsets in cases:
        assert post.shape[1] == 65 and len(seq) >= M, name
        if bsets is None:
            forms |= {map_form(post, seq, None, v, M=M) for v in (True, False)}
            continue
        for bname, (lo, hi) in bsets:
            if R.are_bounds_sane(_sp(lo), _sp(hi), post.shape[0], len(seq)):
                forms |= {map_form(post, seq, (lo, hi), v, M=M) for v in (True, False)}
                n_sane += len(seq) > M
    capfd.readouterr()
    # every dense form, both homes (the control at M is the LDS one); the tiled forms need the engine
    assert forms == {(v, b, False, h) for v in (True, False) for b in (True, False) for h in (True, False)}
    print("sane banded scratch cases: %d" % n_sane)
    assert n_sane >= 12
    free = [c for c in cases if c[4] is None]
    band = [c for c in cases if c[4] is not None]
    for L in lens:
        nbs = [c[1].shape[0] for c in free if len(c[2]) == L and c[1].shape[0] <= 41]
        assert len(nbs) == 2 and (nbs[0] + nbs[1]) % 2 == 1, L                   # both ping-pong parities
        assert any(len(c[2]) == L for c in band), L
    assert {c[1].shape[0] for c in free} == set(SCRATCH_NBLOCK) | {SCRATCH_BAND_NBLOCK}
    assert {c[3] for c in free} == set(PENS) and {c[3] for c in band} == set(PENS)
    assert any(len(c[2]) == M + 1 and c[1].shape[0] > M // 2 for c in free)       # a long walk just above the threshold
    ride = [c for c in cases if c[0].endswith("_ride")]
    assert sorted(len(c[2]) for c in ride) == [M, M + 1]
    for name, post, seq, pens, bsets in ride:
        for bname, (lo, hi) in bsets:
            assert R.are_bounds_sane(_sp(lo), _sp(hi), post.shape[0], len(seq)), (name, bname)
            assert int(np.sum(np.diff(lo.astype(np.int64)) == 1)) == len(seq) - 1       # every move is a step into the lowest cell
            # the alignment sets the score, not the banded forms' START -> END of block 0 and END from there on
            chain = -pens[2] + float(np.sum(np.maximum(-pens[2], post[1:, -1].astype(np.float64))))
            assert float(call_map(R, post, seq, pens, True, (lo, hi))[0]) > chain + 1000, (name, bname)
    capfd.readouterr()


def check_scratch_plan(kind, sizes, counts, in_lds, need):
    """the planner's scratch layout of one launch (sa.plan_scratch): LDS reads take none; every other read's rows,
    need(size) floats from its offset, start on a 16-byte boundary, lie behind the previous read's and inside the
    allocation"""
    off, total = sa.plan_scratch(kind, sizes, counts)
    end = 0
    for i, (n, o) in enumerate(zip(sizes, off)):
        if in_lds(n):
            assert o == -1, (kind, i, n, o)
            continue
        assert o >= end and o % 4 == 0, (kind, i, n, int(o), end)
        end = int(o) + need(n)
    assert end <= total and total % 4 == 0, (kind, end, total)
    assert total <= end + 3 * sum(1 for n in sizes if not in_lds(n)), (kind, end, total)      # rounding only, no more


def test_scratch_plan_keeps_neighbours_apart():
    """plan_add: k_map touches 2 (L + 2) floats from a read's scratch offset (both rows with START and END).  Odd and even
    L just above the threshold and every length of scratch_seqlens, LDS reads between them, several orders."""
    M = lds_max_seq()
    lens = [M + 1, M + 2, 7, M + 3, M + 4, M, M + 1] + list(scratch_seqlens(M)) + [M - 1, M + 5, M + 6, 65536]
    rng = np.random.default_rng(23)
    for order in (np.arange(len(lens)), np.arange(len(lens))[::-1], rng.permutation(len(lens)), rng.permutation(len(lens))):
        L = [lens[i] for i in order]
        check_scratch_plan("map", L, [1 + (i % 41) for i in range(len(L))], lambda n: n <= M, lambda n: 2 * (n + 2))
    for L in (M + 1, M + 2, M + 3, M + 4):                    # a lone read: the allocation covers it
        check_scratch_plan("map", [L], [40], lambda n: n <= M, lambda n: 2 * (n + 2))


@pytest.mark.parametrize("viterbi", [True, False])
def test_restatement_equals_reference_scratch_cases(viterbi):
    """as test_restatement_equals_reference on map_scratch_cases"""
    R = ref_decode_lib()
    if R is None:
        pytest.skip("oracle/_ref/libref_decode.so not built")
    for name, post, seq, pens, bsets in map_scratch_cases():
        if bsets is None:
            want_s, want_p = call_map(R, post, seq, pens, viterbi)
            got_s, got_p = np_map(post, seq, *pens, viterbi=viterbi)
            if viterbi:
                assert np.float32(got_s).tobytes() == want_s.tobytes(), name
                assert np.array_equal(got_p, want_p), name
            else:
                assert abs(float(got_s) - float(want_s)) <= 1e-5 * abs(float(want_s)) + 1e-4, name
            continue
        for bname, bands in bsets:
            if not _sane(bands[0], bands[1], post.shape[0], len(seq)):
                continue
            want_s, _ = call_map(R, post, seq, pens, viterbi, bands)
            got_s, _ = np_map(post, seq, *pens, viterbi=viterbi, low=bands[0], high=bands[1])
            if viterbi:
                assert np.float32(got_s).tobytes() == want_s.tobytes(), (name, bname)
            else:
                assert abs(float(got_s) - float(want_s)) <= 1e-5 * abs(float(want_s)) + 1e-4, (name, bname)


def test_map_post_to_sequence_arguments():
    """scrappy's argument errors and its diagonal band (python/scrappy/__init__.py:522-562), before any GPU work"""
    post = sa.ScrappyMatrix.from_numpy(np.log(np.full((10, 1025), 1.0 / 1025, dtype=np.float32)), sloika=False)
    with pytest.raises(ValueError):
        sa.map_post_to_sequence(post, "ACGTACGTAC", viterbi=False, path=True)
    with pytest.raises(TypeError):
        sa.map_post_to_sequence(np.zeros((10, 1025), dtype=np.float32), "ACGTACGTAC")
    with pytest.raises(ValueError):
        sa.map_post_to_sequence(post, "ACGTACGTACGT", bands=(1, 2, 3))
    bad = (np.ones(10, dtype=np.uintp), np.full(10, 8, dtype=np.uintp))          # low[0] != 0
    with pytest.raises(ValueError):
        sa.map_post_to_sequence(post, "ACGTACGTACGT", bands=bad)
    for nblock, seq_len, w in ((10, 8, 2), (37, 400, 5), (800, 123, 3), (5, 3, 1)):
        gradient = seq_len / nblock
        hband = (2 * w * gradient) / 2
        lo = np.array([max(0, x * gradient - hband) for x in range(nblock)], dtype=np.uintp)
        hi = np.array([min(seq_len, x * gradient + hband) for x in range(nblock)], dtype=np.uintp)
        got = sa.diagonal_bands(w, nblock, seq_len)
        assert got[0].dtype == np.uintp and np.array_equal(got[0], lo) and np.array_equal(got[1], hi)


def test_pyscrap_map_cdef_links(tmp_path):
    """include/pyscrap_map.h: the cdef text of python/pyscrap.h:41-58 and :61, which routes scrappy.map_post_to_sequence
    to this library; every prototype must agree with scrappie_hip.h and link against the built library alone"""
    import re
    text = open(os.path.join(ROOT, "include", "pyscrap_map.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    names = re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*\(", text)
    assert sorted(names) == sorted(["are_bounds_sane", "map_to_sequence_forward", "map_to_sequence_forward_banded",
                                    "map_to_sequence_viterbi", "map_to_sequence_viterbi_banded", "encode_bases_to_integers"])
    src = tmp_path / "link.c"
    src.write_text('#include "scrappie_hip.h"\n' + text + "\nvoid *table[] = {" + ", ".join("(void *)" + n for n in names) +
                   "};\nint main(void) { return table[0] == 0; }\n")
    exe = tmp_path / "link"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", os.path.join(ROOT, "scrappie_amd"), "-lscrappie_hip",
                        "-Wl,-rpath," + os.path.join(ROOT, "scrappie_amd")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


FA_SHA256 = {
    "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch174_read172_strand":
        "0dcf90a5b480a0765f5090e4c888a946330a956aad9cc2596f53e474ad0a2786",
    "MINICOL228_20161012_FNFAB42578_MN17976_mux_scan_HG_52221_ch271_read66_strand":
        "e56d9dc82d910b61ed30656ebb6035fefc029da2a675025eaa0f90b7a7e7e6b4",
}


def test_fasta_fixtures():
    """tests/golden/reads/*.fa: the reference's reads/*.fa of the two bundled reads that have one, byte for byte (checked
    against the reference checkout where it exists, as oracle/Makefile finds it)"""
    import hashlib
    ref_reads = os.path.join(os.environ.get("REF", "/root/reference"), "reads")
    for name, sha in FA_SHA256.items():
        data = open(os.path.join(ROOT, "tests", "golden", "reads", name + ".fa"), "rb").read()
        assert hashlib.sha256(data).hexdigest() == sha
        if os.path.exists(os.path.join(ref_reads, name + ".fa")):
            assert open(os.path.join(ref_reads, name + ".fa"), "rb").read() == data


def test_seqmappy_cli_without_gpu(tmp_path):
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.join(ROOT, "scrappie_amd", "csrc"), "all"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([CLI, "help"], capture_output=True, text=True)
    assert r.returncode == 0 and "seqmappy" in r.stdout
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGT\nACGT\n")
    r = subprocess.run([CLI, "seqmappy", str(fa)], capture_output=True, text=True)
    assert r.returncode != 0 and "fast5 file is a required argument" in r.stderr
    if sa.lib().scrappie_hip_device_count() > 0:
        return
    r = subprocess.run([CLI, "seqmappy", str(fa), os.path.join(ROOT, "tests", "golden", "reads", "read_ch228_file118.i16")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "HIP device" in r.stderr
