"""The cut of the split products on the device (run with -m gpu on an MI355X), through the C ABI.

Every activation that enters a split product is scaled by 64 and cut into two fp16 pieces (sh_kernels.h: split_pair / split8):
p1 = fp16(64 x), p2 = fp16(64 x - p1).  The kernels form p2 with one mixed-precision fused multiply-add per value that reads p1's half
directly (v_fma_mixlo_f16 / v_fma_mixhi_f16) instead of going back through fp32; the residual is exact in fp32, so both round the same
value once and the bits must be those of the definition:

  * scrappie_hip_debug_split (split8 on consecutive groups of eight) against numpy's statement of the definition, uint16 against uint16,
    on the inputs where a rounding could part ways: every fp16 tie point / 64 with both of its fp32 neighbours, signed zeros, fp32
    subnormals, the limits of the operand range, and seeded normals at scales 1, 1e-3, 1e-6 and uniforms in +-1000;
  * one small ragged batch end to end (two tiles of 16 reads in one workgroup of the recurrent layers, lanes of padding reads and reads
    that have ended in both the recurrence team's publish and the projection team's split8): no expectation is committed at this size,
    so every call is the oracle's integer decode of the engine's own posterior of that read, bit for bit, and that posterior is within
    tests/test_gpu_parity.py's fp32 tolerances of the same network on the exact-fp32 kernels (debug option force_f32_layers).
"""
import numpy as np
import pytest

import scrappie_amd as sa
from scrappie_amd import model, synth

from test_gpu_parity import P_TOL, LOGP_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = sa.Engine(0)
    yield e
    e.close()


def _definition(x):
    """sh_kernels.h: xs = 64 x; p1 = fp16(xs) (round to nearest even); p2 = fp16(xs - p1)."""
    xs = np.float32(x) * np.float32(64)
    p1 = xs.astype(np.float16)
    p2 = (xs - p1.astype(np.float32)).astype(np.float16)
    return p1.view(np.uint16), p2.view(np.uint16)


def _inputs():
    f32 = np.float32
    # every tie point of fp16 (half way between two consecutive finite values, exact in fp32) brought back by the scale,
    # with the fp32 value on either side of it
    grid = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(f32)
    ties = ((grid[:-1] + grid[1:]) * f32(0.5)) / f32(64)
    ties = np.concatenate([ties, np.nextafter(ties, f32(np.inf)), np.nextafter(ties, f32(-np.inf))]).astype(f32)
    tiny = np.array([1, 2, 3, 0x1234, 0x3FFFFF, 0x400000, 0x7FFFFF, 0x800000], dtype=np.uint32).view(f32)      # fp32 subnormals, and the first normal
    edge = np.array([0.0, 999.99994, 1023.0, 1.0, 2.0 ** -14 / 64, 2.0 ** -24 / 64, 2.0 ** -25 / 64], dtype=f32)
    special = np.concatenate([ties, tiny, edge])
    special = np.concatenate([special, -special])
    rng = np.random.default_rng(20240611)
    parts = [special]
    for scale in (1.0, 1e-3, 1e-6):
        parts.append((rng.standard_normal(1000000) * scale).astype(f32))
    parts.append(rng.uniform(-1000.0, 1000.0, 1000000).astype(f32))
    x = np.concatenate(parts)
    assert np.all(np.isfinite(x)) and np.max(np.abs(x)) < 1023.75      # NaN and what 64 x rounds past fp16's largest value are not operands
    return x, len(special)


def test_cut_is_the_definition_bit_for_bit(eng):
    x, nspecial = _inputs()
    w1, w2 = _definition(x)
    # the premise of the one-rounding form, on this very set: the residual is exact in fp32
    xs = x * np.float32(64)
    p1 = w1.view(np.float16)
    assert np.array_equal((xs - p1.astype(np.float32)).astype(np.float64), xs.astype(np.float64) - p1.astype(np.float64))
    g1, g2 = eng.debug_split(x)
    bad1, bad2 = np.flatnonzero(g1 != w1), np.flatnonzero(g2 != w2)
    print("%d values (%d ties, zeros, subnormals and limits): p1 differs at %d, p2 at %d" % (len(x), nspecial, len(bad1), len(bad2)))
    for b in bad2[:8]:
        print("  x = %r (%#010x): p2 %#06x, definition %#06x (p1 %#06x)" % (float(x[b]), int(x[b:b + 1].view(np.uint32)[0]), int(g2[b]), int(w2[b]), int(g1[b])))
    assert len(bad1) == 0 and len(bad2) == 0
    # a length that is no multiple of eight: the last group is padded, not read past
    g1, g2 = eng.debug_split(x[:13])
    assert np.array_equal(g1, w1[:13]) and np.array_equal(g2, w2[:13])


def test_small_ragged_batch_end_to_end(eng):
    import oracle
    w = model.synthetic_model("rgrgr_r94", seed=11)
    eng.load_model("cut_split", w)
    eng.debug_option("force_f32_layers", 1)
    eng.load_model("cut_exact", w)
    eng.debug_option("force_f32_layers", 0)
    lens = [400 + (i * 131) % 401 for i in range(32)]                  # 400 .. 800 samples, no two tiles alike
    sigs = [synth.medmad_normalise(synth.synthetic_signal(n, 8100 + i)) for i, n in enumerate(lens)]
    p = eng.default_params(want_pos=1, local_pen=120.0)
    try:
        eng.debug_option("gru_tiles", 2)
        calls = eng.basecall(sigs, "cut_split", p)
        assert int(eng.debug_fetch("gru_tiles", np.int32)[0]) == 2
    finally:
        eng.debug_option("gru_tiles", 0)
    worst_p = worst_logp = 0.0
    for x, c in zip(sigs, calls):
        post = eng.posterior(x, "cut_split", min_prob=p.min_prob)
        sc, seq = oracle.decode_transducer(post, p.stay_pen, p.skip_pen, p.local_pen, False)
        rc, seq = oracle.homopolymer_path(post, seq)
        bases, pos = oracle.overlapper(seq, 1024)
        assert c is not None and c["nblock"] == post.shape[0]
        assert c["bases"] == bases and np.float32(c["score"]) == np.float32(sc) and list(c["pos"]) == list(pos)
        want = eng.posterior(x, "cut_exact", min_prob=p.min_prob)
        pg, pw = np.exp(post.astype(np.float64)), np.exp(want.astype(np.float64))
        big = pw > 1e-4
        worst_p, worst_logp = max(worst_p, float(np.max(np.abs(pg - pw)))), max(worst_logp, float(np.max(np.abs(post[big] - want[big]))))
    print("32 reads of %d .. %d samples: posterior against the exact-fp32 kernels max |dp| %.3g, max |dlogp| %.3g" % (min(lens), max(lens), worst_p, worst_logp))
    assert worst_p <= P_TOL and worst_logp <= LOGP_TOL
