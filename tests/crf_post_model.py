"""What the tests of the batched CRF posterior share (tests/test_crf_post_cpu.py, tests/test_gpu_crf_post.py): a float64 restatement of
posterior_crf's forward / backward pass (decode.c:928-1012) with its extra e^0 in every column total (quirk Q16), the five input families,
the host function on them, and the bound the device is held to."""

import numpy as np

import scrappie_amd as sa

BLOCKS = (1, 2, 7, 8, 9, 15, 16, 17, 100, 800)      # the ring's (8) and the tile's (16) edges, a single block, one production-sized read
NREAD = 33                                           # two full tiles and one lane of a third
FAMILIES = ("normal", "peaked", "underflow", "shifted", "tie")


def block_counts(seed=7):
    """every length of BLOCKS once (one read of 800 blocks), the other 23 drawn from the short ones"""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.permutation(list(BLOCKS) + list(rng.choice(BLOCKS[:-1], NREAD - len(BLOCKS))))]


def family(name, seed=11):
    """33 float32 transition matrices (nblock, 25), entry to * 5 + from"""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    out = []
    for T in block_counts():
        a = rng.standard_normal((T, 25))
        if name == "peaked":          # one transition per block at +20, the rest at -20
            a = np.full((T, 25), -20.0)
            a[np.arange(T), rng.integers(0, 25, T)] = 20.0
        elif name == "underflow":     # a random third at -1e4, and in some blocks every transition into one state
            a[rng.random((T, 25)) < 1.0 / 3.0] = -1e4
            for t in np.nonzero(rng.random(T) < 0.1)[0]:
                to = int(rng.integers(0, 5))
                a[t, 5 * to:5 * to + 5] = -1e4
        elif name == "shifted":       # messages grow by about 5 a block: an un-normalised input
            a = a + 3.0
        elif name == "tie":           # all 25 equal: every state gets the same value
            a = np.full((T, 25), float(rng.standard_normal()))
        out.append(np.ascontiguousarray(a, dtype=np.float32))
    return out


def model_f64(mats):
    """float64 forward / backward over every matrix of the list at once (padded to the longest): a list of (nblock + 1, 5) arrays"""
    R, Tmax = len(mats), max(len(m) for m in mats)
    T = np.array([len(m) for m in mats])
    tr = np.zeros((R, Tmax, 5, 5))
    for r, m in enumerate(mats):
        tr[r, :len(m)] = np.asarray(m, dtype=np.float64).reshape(-1, 5, 5)          # [to][from]
    alpha = np.zeros((R, Tmax + 1, 5))
    for t in range(Tmax):
        alpha[:, t + 1] = np.logaddexp.reduce(tr[:, t] + alpha[:, t, None, :], axis=2)
    post = np.zeros((R, Tmax + 1, 5))
    beta = np.zeros((R, 5))
    idx = np.arange(R)
    post[idx, T] = alpha[idx, T]
    for t in range(Tmax - 1, -1, -1):
        new = np.logaddexp.reduce(tr[:, t] + beta[:, :, None], axis=1)               # over `to`
        beta = np.where((t < T)[:, None], new, 0.0)
        post[:, t] = alpha[:, t] + beta
    tot = np.logaddexp(0.0, np.logaddexp.reduce(post, axis=2))                       # Q16: the total starts at 0.0, an extra e^0
    prob = np.exp(post - tot[:, :, None])
    return [prob[r, :T[r] + 1] for r in range(R)]


def host_posterior(mat):
    """the library's per-read posterior_crf (pinned to the compiled reference) on one (nblock, 25) array"""
    m = sa.ScrappyMatrix.from_numpy(mat, sloika=False)
    bp = sa.lib().posterior_crf(m.data())
    assert bp
    return sa.ScrappyMatrix(bp).data(as_numpy=True, sloika=False)


def max_err(got, want):
    return max(float(np.max(np.abs(np.asarray(g, dtype=np.float64) - w))) for g, w in zip(got, want))


def reference(name):
    """(matrices, float64 model, e_ref, e_ref of every read) of a family: e_ref is the host function's own maximum absolute error,
    computed every run"""
    mats = family(name)
    want = model_f64(mats)
    host = [host_posterior(m) for m in mats]
    assert all(np.all(np.isfinite(h)) for h in host), name
    per_read = [max_err([h], [w]) for h, w in zip(host, want)]
    return mats, want, max(per_read), per_read


def bound(e_ref):
    """Both implementations round once per log-sum-exp in the same order; the device's log-sum-exp adds at most about 3 ulp of its
    correction term (<= log 2) where libm adds 1, so a step's error is within 3 x the host's wherever the term matters, and 4 leaves a
    step of slack.  The 1e-6 floor covers the final exponential on values <= 1 and the families where the host happens to be nearly exact."""
    return 4.0 * e_ref + 1e-6
