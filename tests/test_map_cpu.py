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
