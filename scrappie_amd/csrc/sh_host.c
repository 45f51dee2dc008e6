/* sh_host.c -- host-side C of libscrappie_hip.so.
 *
 * The reference keeps its whole path in C on the host; here only the parts that
 * are O(read length) integer/byte work or one-off signal preparation stay on the
 * host, written in C and
 * exported with the reference's own names so existing bindings keep working.
 * Everything numeric per block runs in the HIP kernels (scrappie_hip.hip).
 *
 * Citations: file:line under /root/reference/src.
 */
#define _POSIX_C_SOURCE 200809L
#include "scrappie_hip.h"
#include "sh_internal.h"

#include <err.h>
#include <math.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ */
/* matrix container (scrappie_matrix.c:11, :69, :130)                  */
/* ------------------------------------------------------------------ */
scrappie_matrix make_scrappie_matrix(size_t nr, size_t nc) {
    if (nr == 0 || nc == 0) return NULL;
    const size_t nrq = (nr + 3) / 4;
    if (nc != 0 && (nrq * 16) > ((size_t)-1) / nc) return NULL;   /* overflow */
    scrappie_matrix m = malloc(sizeof(*m));
    if (!m) return NULL;
    void *buf = NULL;
    if (posix_memalign(&buf, 16, nrq * 16 * nc) != 0) {
        free(m);
        return NULL;
    }
    memset(buf, 0, nrq * 16 * nc);
    m->nr = nr; m->nrq = nrq; m->nc = nc; m->stride = 4 * nrq;
    m->data.v = buf;
    return m;
}

scrappie_matrix mat_from_array(const float *x, size_t nr, size_t nc) {
    if (!x) return NULL;
    scrappie_matrix m = make_scrappie_matrix(nr, nc);
    if (!m) return NULL;
    for (size_t c = 0; c < nc; c++)
        memcpy(m->data.f + c * m->stride, x + c * nr, nr * sizeof(float));
    return m;
}

scrappie_matrix free_scrappie_matrix(scrappie_matrix mat) {
    if (mat) {
        free(mat->data.v);
        free(mat);
    }
    return NULL;
}

/* ------------------------------------------------------------------ */
/* P0: order statistics by selection instead of the reference's qsort  */
/* (util.c:92-130).  The two order statistics a quantile needs are the */
/* same values whichever way they are found, so results are identical. */
/* ------------------------------------------------------------------ */
static inline void swapf(float *a, float *b) { float t = *a; *a = *b; *b = t; }

/* after return v[k] is the k-th smallest and v[k+1..n) >= v[k] */
static void select_kth(float *v, size_t n, size_t k) {
    size_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (v[mid] < v[lo]) swapf(&v[mid], &v[lo]);
        if (v[hi] < v[lo]) swapf(&v[hi], &v[lo]);
        if (v[hi] < v[mid]) swapf(&v[hi], &v[mid]);
        const float pivot = v[mid];
        size_t i = lo, j = hi;
        while (i <= j) {
            while (v[i] < pivot) i++;
            while (v[j] > pivot) j--;
            if (i <= j) {
                swapf(&v[i], &v[j]);
                i++;
                if (j == 0) break;
                j--;
            }
        }
        if (k <= j) hi = j;
        else if (k >= i) lo = i;
        else return;
    }
}

/* one quantile of x[0..n) using caller scratch (n floats); util.c:117-125 */
static float quantile_scratch(const float *x, size_t n, float p, float *scratch) {
    memcpy(scratch, x, n * sizeof(float));
    const size_t idx = (size_t)(p * (n - 1));
    const float remf = p * (n - 1) - idx;
    select_kth(scratch, n, idx);
    const float a = scratch[idx];
    if (idx < n - 1) {
        float b = scratch[idx + 1];
        for (size_t i = idx + 2; i < n; i++) if (scratch[i] < b) b = scratch[i];
        return (float)((1.0 - remf) * a + remf * b);
    }
    return a;
}

float sh_medianf(const float *x, size_t n, float *scratch) {
    return quantile_scratch(x, n, 0.5f, scratch);
}

/* util.c:156-180; scratch holds 2n floats */
float sh_madf(const float *x, size_t n, const float *med, float *scratch) {
    const float mad_scaling_factor = 1.4826;
    if (n == 1) return 0.0f;
    const float m = med ? *med : sh_medianf(x, n, scratch);
    float *absdiff = scratch + n;
    for (size_t i = 0; i < n; i++) absdiff[i] = fabsf(x[i] - m);
    return sh_medianf(absdiff, n, scratch) * mad_scaling_factor;
}

/* util.c:190-205 */
void medmad_normalise_array(float *x, size_t n) {
    if (!x || n == 0) return;
    if (n == 1) { x[0] = 0.0f; return; }
    float *scratch = malloc(2 * n * sizeof(float));
    if (!scratch) return;
    const float xmed = sh_medianf(x, n, scratch);
    const float xmad = sh_madf(x, n, &xmed, scratch);
    for (size_t i = 0; i < n; i++) x[i] = (x[i] - xmed) / xmad;
    free(scratch);
}

/* scrappie_common.c:39-73 */
raw_table trim_raw_by_mad(raw_table rt, size_t chunk_size, float perc) {
    const size_t nsample = rt.end - rt.start;
    const size_t nchunk = nsample / chunk_size;
    rt.end = nchunk * chunk_size;            /* relative to 0, as the reference (Q14) */
    if (nchunk == 0) return rt;
    float *madarr = malloc(nchunk * sizeof(float));
    float *scratch = malloc(2 * (chunk_size > nchunk ? chunk_size : nchunk) * sizeof(float));
    if (!madarr || !scratch) {
        free(madarr); free(scratch);
        return (raw_table){0};
    }
    for (size_t i = 0; i < nchunk; i++)
        madarr[i] = sh_madf(rt.raw + rt.start + i * chunk_size, chunk_size, NULL, scratch);
    const float thresh = quantile_scratch(madarr, nchunk, perc, scratch);
    for (size_t i = 0; i < nchunk; i++) {
        if (madarr[i] > thresh) break;
        rt.start += chunk_size;
    }
    for (size_t i = nchunk; i > 0; i--) {
        if (madarr[i - 1] > thresh) break;
        rt.end -= chunk_size;
    }
    free(scratch);
    free(madarr);
    return rt;
}

/* scrappie_common.c:5-21; like the reference, frees rt.raw when the trimmed
 * window is empty */
raw_table trim_and_segment_raw(raw_table rt, size_t trim_start, size_t trim_end,
                               size_t varseg_chunk, float varseg_thresh) {
    if (!rt.raw) return (raw_table){0};
    rt = trim_raw_by_mad(rt, varseg_chunk, varseg_thresh);
    if (!rt.raw) return (raw_table){0};
    rt.start = (rt.n - rt.start) > trim_start ? rt.start + trim_start : rt.n;
    rt.end = (rt.end > trim_end) ? rt.end - trim_end : 0;
    if (rt.start >= rt.end) {
        free(rt.raw);
        return (raw_table){0};
    }
    return rt;
}

/* ------------------------------------------------------------------ */
/* D3 k-mer stitching (decode.c:367-509)                               */
/* ------------------------------------------------------------------ */
static const char BASES[4] = { 'A', 'C', 'G', 'T' };

static inline int kmer_shift(int k1, int k2, int nkmer) {
    /* smallest s >= 1 with suffix_{k-s}(k1) == prefix_{k-s}(k2) */
    int mask = nkmer - 1, s = 0;
    do {
        mask >>= 2;
        k1 &= mask;
        k2 >>= 2;
        s++;
    } while (k1 != k2);
    return s;
}

char *overlapper(const int *seq, size_t n, int nkmer, int *pos) {
    if (!seq) return NULL;
    size_t nbit = 0;
    for (size_t x = (size_t)nkmer; x; x >>= 1) nbit++;
    const size_t klen = nbit / 2;
    size_t first = 0;
    while (first < n && seq[first] < 0) first++;
    if (first == n) return NULL;

    size_t length = klen;
    for (size_t k = first + 1, prev = (size_t)seq[first]; k < n; k++) {
        if (seq[k] < 0) continue;
        length += (size_t)kmer_shift((int)prev, seq[k], nkmer);
        prev = (size_t)seq[k];
    }
    char *bases = calloc(length + 1, 1);
    if (!bases) return NULL;
    for (size_t kmer = (size_t)seq[first], i = klen; i-- > 0; kmer >>= 2)
        bases[i] = BASES[kmer & 3];
    if (pos) pos[0] = 0;
    size_t tail = klen - 1;
    int prev = seq[first];
    for (size_t k = first + 1; k < n; k++) {
        if (seq[k] < 0) {
            if (pos) pos[k] = pos[k - 1];
            continue;
        }
        const int s = kmer_shift(prev, seq[k], nkmer);
        if (pos) pos[k] = pos[k - 1] + s;
        prev = seq[k];
        size_t kmer = (size_t)seq[k];
        for (int i = 0; i < s; i++, kmer >>= 2)
            bases[tail + (size_t)(s - i)] = BASES[kmer & 3];
        tail += (size_t)s;
    }
    return bases;
}

/* decode.c:895-918 (pos is accepted and left untouched, as there: Q11) */
char *crfpath_to_basecall(int const *path, size_t npos, int *pos) {
    if (!path || !pos) return NULL;
    size_t nb = 0;
    for (size_t i = 0; i < npos; i++) nb += (path[i] < 4);
    char *out = calloc(nb + 1, 1);
    if (!out) return NULL;
    for (size_t i = 0, j = 0; i < npos; i++)
        if (path[i] < 4) out[j++] = BASES[path[i]];
    return out;
}

/* ------------------------------------------------------------------ */
/* Dwell correction of homopolymer lengths (decode.c:511-702): the last */
/* step of `scrappie events`.  The host statement the device form       */
/* (sh_dwell.h) is held against, and what re-stitches a read that did   */
/* not fit its reservation on the device.                               */
/* ------------------------------------------------------------------ */
static int kmer_is_homopolymer(int kmer, int klen) {
    for (int i = 1; i < klen; i++)
        if (((kmer >> (2 * i)) & 3) != (kmer & 3)) return 0;
    return 1;
}

/* bases a homopolymer that was dwelt in for hdwell samples is given: a float division, then round half away from zero
 * (decode.c:511-514).  0 where the count is no int (a scale of zero, a NaN): the reference is undefined there. */
static int dwell_bases(int hdwell, int homo, const dwell_model *dm, int *count) {
    const float q = roundf(((float)hdwell - dm->base_adj[homo & 3]) / dm->scale);
    if (!(q >= 0.0f && q < 1073741824.0f)) return 0;
    *count = (int)q;
    return 1;
}

/* One forward walk over the path, as the reference's length pass and fill pass both are.  Returns what strlen gives on the
 * reference's string and writes those bytes when out is not NULL; -1 where the reference is undefined (no k-mer at all, a
 * count that is no int).  A homopolymer is entered at a k-mer behind the first only; stays and repeats of its k-mer add
 * their dwell while it lasts; leaving it emits its bases in front of the next k-mer's.  The last homopolymer's fill starts
 * one byte early (decode.c:633-635, on the base it repeats), so where it has bases the string ends one short of them. */
static long dwell_walk(const int *seq, const int *dwell, int n, int nkmer, const dwell_model *dm, char *out) {
    int klen = 0;
    for (int x = nkmer; x > 1; x >>= 2) klen++;
    int first = 0;
    while (first < n && seq[first] < 0) first++;
    if (first >= n) return -1;
    long len = 0;
    for (int i = klen - 1; i >= 0; i--, len++)
        if (out) out[len] = BASES[(seq[first] >> (2 * i)) & 3];
    int prev = seq[first], homo = -1, hdwell = 0, cnt = 0;
    for (int k = first + 1; k < n; k++) {
        const int cur = seq[k];
        if (cur < 0 || cur == homo) {
            if (homo >= 0) hdwell += dwell[k];
            continue;
        }
        if (homo >= 0) {
            if (!dwell_bases(hdwell, homo, dm, &cnt)) return -1;
            for (int i = 0; i < cnt; i++, len++)
                if (out) out[len] = BASES[homo & 3];
            homo = -1;
            hdwell = 0;
        }
        const int s = kmer_shift(prev, cur, nkmer);
        for (int i = s - 1; i >= 0; i--, len++)
            if (out) out[len] = BASES[(cur >> (2 * i)) & 3];
        prev = cur;
        if (kmer_is_homopolymer(cur, klen)) {
            homo = cur;
            hdwell = dwell[k];
        }
    }
    if (homo >= 0) {
        if (!dwell_bases(hdwell, homo, dm, &cnt)) return -1;
        for (int i = 0; i + 1 < cnt; i++, len++)
            if (out) out[len] = BASES[homo & 3];
    }
    return len;
}

char *dwell_corrected_overlapper(const int *seq, const int *dwell, int n, int nkmer, const dwell_model dm) {
    if (!seq || !dwell || n <= 0 || nkmer < 4) return NULL;
    const long len = dwell_walk(seq, dwell, n, nkmer, &dm, NULL);
    if (len < 0) return NULL;
    char *bases = calloc((size_t)len + 2, 1);
    if (!bases) return NULL;
    (void)dwell_walk(seq, dwell, n, nkmer, &dm, bases);
    return bases;
}

/* decode.c:661-693: the mean dwell of the steps outside homopolymers, with the prior as one more observation.  pos / state:
 * n ints each, `stride` bytes apart.  The sums are ints; prior + sum is a float addition, the division a double one, rounded
 * to float once. */
float sh_dwell_scale(const void *pos, const void *state, size_t stride, const int *dwell, int n, float prior_num, size_t basecall_len) {
    int tot_step_dwell = 0, nstep = 0;
    for (int ev = 0, ppos = -2, evdwell = 0, pstate = -1; ev < n; ev++) {
        const int p = *(const int *)((const char *)pos + (size_t)ev * stride);
        const int s = *(const int *)((const char *)state + (size_t)ev * stride);
        if (p == ppos) { evdwell += dwell[ev]; continue; }
        if (p == ppos + 1 && s != pstate) { tot_step_dwell += evdwell; nstep++; }
        evdwell = dwell[ev];
        ppos = p;
        pstate = s;
    }
    const float prior_scale = prior_num / (float)basecall_len;
    const float num = prior_scale + (float)tot_step_dwell;
    return (float)((double)num / (1.0 + (double)nstep));
}

/* the float numerator of the prior: the last event's length + (float)(the span of the starts) (decode.c:689-692) */
float sh_dwell_prior_num(const event_t *ev, size_t n) {
    return ev[n - 1].length + (float)(ev[n - 1].start - ev[0].start);
}

static int *event_dwells(const event_t *ev, size_t n) {
    int *dwell = malloc((n ? n : 1) * sizeof(int));
    if (dwell)
        for (size_t i = 0; i < n; i++) dwell[i] = (int)ev[i].length;
    return dwell;
}

float scrappie_hip_dwell_scale(const event_table et, size_t basecall_len) {
    if (!et.event || et.end <= et.start || et.end > et.n || basecall_len == 0) return NAN;
    const event_t *ev = et.event + et.start;
    const size_t n = et.end - et.start;
    int *dwell = event_dwells(ev, n);
    if (!dwell) return NAN;
    const float scale = sh_dwell_scale(&ev[0].pos, &ev[0].state, sizeof(event_t), dwell, (int)n, sh_dwell_prior_num(ev, n), basecall_len);
    free(dwell);
    return scale;
}

char *homopolymer_dwell_correction(const event_table et, const int *seq, size_t nstate, size_t basecall_len) {
    if (!et.event || !seq || et.end <= et.start || et.end > et.n || basecall_len == 0 || nstate < 5) return NULL;
    const event_t *ev = et.event + et.start;
    const size_t n = et.end - et.start;
    if (n > (size_t)INT32_MAX) return NULL;
    int *dwell = event_dwells(ev, n);
    if (!dwell) return NULL;
    const dwell_model dm = { sh_dwell_scale(&ev[0].pos, &ev[0].state, sizeof(event_t), dwell, (int)n, sh_dwell_prior_num(ev, n), basecall_len),
                             { 0.0f, 0.0f, 0.0f, 0.0f } };
    char *bases = dwell_corrected_overlapper(seq, dwell, (int)n, (int)nstate - 1, dm);
    free(dwell);
    return bases;
}

/* The same on a read the engine holds as arrays: a path of n + ntrail entries (the decoder's; `scrappie events` stitches its
 * first n, one per event), n dwells, the prior's numerator.  pos_out (may be NULL): n + ntrail ints, overlapper's.  Returns the corrected call, or the plain one where the correction has none; NULL: no k-mer. */
char *sh_dwell_stitch(const int *path, const int *dwell, int n, int ntrail, int nstate, float prior_num, int *pos_out) {
    const size_t nall = (size_t)n + (size_t)ntrail;
    int *pos = calloc(2 * nall + 2, sizeof(int));
    if (!pos) return NULL;
    int *state = pos + nall + 1;
    char *plain = overlapper(path, nall, nstate - 1, pos);
    if (!plain) { free(pos); return NULL; }
    for (int i = 0; i < n; i++) state[i] = 1 + path[i];
    const dwell_model dm = { sh_dwell_scale(pos, state, sizeof(int), dwell, n, prior_num, strlen(plain)), { 0.0f, 0.0f, 0.0f, 0.0f } };
    char *bases = dwell_corrected_overlapper(path, dwell, n, nstate - 1, dm);
    if (pos_out) memcpy(pos_out, pos, nall * sizeof(int));
    free(pos);
    if (!bases) return plain;
    free(plain);
    return bases;
}

/* ------------------------------------------------------------------ */
/* D2 homopolymer correction (homopolymer.c:67-235) on a 5-row side     */
/* buffer: side[t*5 + {0..3}] = log-posterior of the homopolymer k-mer  */
/* of base A,C,G,T at block t, side[t*5 + 4] = stay.  Only those five   */
/* rows are ever read by the reference (homopolymer.c:200,209-210).     */
/* ------------------------------------------------------------------ */
static inline int repeat_kmer(int b, int k) {   /* scrappie_seq_helpers.c:115 */
    int y = 0;
    for (int i = 0; i < k; i++) y = y * 4 + b;
    return y;
}

int sh_kmerlength(int nstate) {                 /* scrappie_seq_helpers.c:132 */
    return (int)(logf((float)nstate) / logf(4.0f));
}

int sh_homopolymer_side(const float *side, int *path, int nblock, int nstate) {
    const int klen = sh_kmerlength(nstate);
    const int fkm1 = 1 << (2 * (klen - 1)), fkm2 = 1 << (2 * (klen - 2));
    const int cap = nblock / 2;
    if (cap <= 0) return 0;
    int *runs = malloc(3 * (size_t)cap * sizeof(int));
    if (!runs) return -1;
    int *rstart = runs, *rlen = runs + cap, *rbase = runs + 2 * cap;
    int nrun = 0;
    /* candidate runs, base by base, in path order (homopolymer.c:95-138) */
    for (int b = 0; b < 4; b++) {
        const int hk = repeat_kmer(b, klen), hk1 = repeat_kmer(b, klen - 1), hk2 = repeat_kmer(b, klen - 2);
        for (int i = 1; i < nblock - 2; i++) {
            const int p = path[i - 1], q = path[i];
            const int q_ok = (q == -1) || (q == hk);
            if (p != -1 && p != hk && (p % fkm1) == hk1 && q_ok) {
                int e = i + 1;
                while (e < nblock && (path[e] == -1 || path[e] == hk)) e++;
                if (nrun < cap) { rstart[nrun] = i; rlen[nrun] = e - i; rbase[nrun] = b; nrun++; }
            }
            if (p != -1 && (p % fkm2) == hk2 && (p % fkm1) != hk1 && q_ok) {
                int j = i;
                while (j < nblock && path[j] == -1) j++;
                if (path[j] == hk && j < nblock - 1) {
                    int e = j + 1;
                    while (e < nblock && (path[e] == -1 || path[e] == hk)) e++;
                    if (nrun < cap) { rstart[nrun] = j; rlen[nrun] = e - j; rbase[nrun] = b; nrun++; }
                }
            }
        }
    }
    /* replace the Viterbi count of each run by the posterior mean count */
    for (int r = 0; r < nrun; r++) {
        const int hk = repeat_kmer(rbase[r], klen);
        const int from = rstart[r], to = from + rlen[r] - 1;
        int nvit = 0;
        double nmean = 0.0;
        for (int i = from; i <= to; i++) {
            const float *s = side + (size_t)(i - 1) * 5;     /* block i-1 pairs with path[i] (Q8) */
            const double ps = expf(s[4]), pr = expf(s[rbase[r]]);
            nmean += pr / (pr + ps);
            nvit += (path[i] == hk);
        }
        const int newn = (int)(nmean + 0.5);
        if (newn != nvit)
            for (int i = 0; i <= to - from; i++) path[from + i] = (i < newn) ? hk : -1;
    }
    free(runs);
    return 0;
}

/* homopolymer.c:175 on a full posterior matrix (per-read surface) */
int homopolymer_path(const_scrappie_matrix post, int *viterbipath,
                     enum homopolymer_calculation flag) {
    if (flag != HOMOPOLYMER_MEAN) return 0;
    if (!post || !viterbipath) return -1;
    const int T = (int)post->nc, ns = (int)post->nr;
    const int klen = sh_kmerlength(ns);
    float *side = malloc((size_t)T * 5 * sizeof(float));
    if (!side) return -1;
    for (int t = 0; t < T; t++) {
        const float *col = post->data.f + (size_t)t * post->stride;
        for (int b = 0; b < 4; b++) side[t * 5 + b] = col[repeat_kmer(b, klen)];
        side[t * 5 + 4] = col[ns - 1];
    }
    const int rc = sh_homopolymer_side(side, viterbipath, T, ns);
    free(side);
    return rc;
}

/* ------------------------------------------------------------------ */
/* D5 posterior_crf (decode.c:928-1012): optional per-block state       */
/* posterior for the CRF model; O(25 T) with libm, kept on the host.    */
/* (Batched, on the device: k_crf_post, sh_crf_post.h; this one is the   */
/* reference's to the bit and stays what the per-read symbol runs.)     */
/* ------------------------------------------------------------------ */
static inline float lse2(float x, float y) {       /* util.h:162 */
    return fmaxf(x, y) + log1pf(expf(-fabsf(x - y)));
}

scrappie_matrix posterior_crf(const_scrappie_matrix trans) {
    if (!trans) return NULL;
    const size_t ns = (size_t)roundf(sqrtf((float)trans->nr));
    const size_t T = trans->nc;
    scrappie_matrix post = make_scrappie_matrix(ns, T + 1);
    float *bwd = malloc(2 * ns * sizeof(float));
    if (!post || !bwd) { free(bwd); return free_scrappie_matrix(post); }
    /* forward messages into post columns 1..T (column 0 stays 0) */
    for (size_t t = 0; t < T; t++) {
        const float *tr = trans->data.f + t * trans->stride;
        const float *a = post->data.f + t * post->stride;
        float *c = post->data.f + (t + 1) * post->stride;
        for (size_t to = 0; to < ns; to++) {
            float acc = tr[to * ns] + a[0];
            for (size_t fr = 1; fr < ns; fr++) acc = lse2(acc, tr[to * ns + fr] + a[fr]);
            c[to] = acc;
        }
    }
    float *prev = bwd, *curr = bwd + ns;
    for (size_t s = 0; s < ns; s++) curr[s] = 0.0f;
    {   /* last column: normalise (accumulator starts at 0.0f like the reference) */
        float *last = post->data.f + T * post->stride, tot = 0.0f;
        for (size_t s = 0; s < ns; s++) tot = lse2(tot, last[s]);
        for (size_t s = 0; s < ns; s++) last[s] = expf(last[s] - tot);
    }
    for (size_t t = T; t-- > 0;) {
        const float *tr = trans->data.f + t * trans->stride;
        float *col = post->data.f + t * post->stride;
        { float *x = curr; curr = prev; prev = x; }
        for (size_t s = 0; s < ns; s++) curr[s] = tr[s] + prev[0];
        for (size_t to = 1; to < ns; to++)
            for (size_t fr = 0; fr < ns; fr++)
                curr[fr] = lse2(curr[fr], tr[to * ns + fr] + prev[to]);
        float tot = 0.0f;
        for (size_t s = 0; s < ns; s++) { col[s] += curr[s]; tot = lse2(tot, col[s]); }
        for (size_t s = 0; s < ns; s++) col[s] = expf(col[s] - tot);
    }
    free(bwd);
    return post;
}

/* The host side of the batched posterior (k_crf_post, sh_eng_crfpost.inc): where every read's (nblock + 1) x 5 floats lie in the output buffer,
 * the staging of a launch's matrices, a result as posterior_crf returns it.  Plain C, so that a sanitizer build can run them (tests/crf_post_asan.c). */
long long scrappie_hip_crf_post_plan(const size_t *nblock, size_t n, long long *off) {
    if (n && (!nblock || !off)) return -1;
    long long tot = 0;
    for (size_t i = 0; i < n; i++) {
        off[i] = tot;
        if (nblock[i]) tot += (long long)((((nblock[i] + 1) * 5) + 3) & ~(size_t)3);      /* starts stay 16-byte aligned; no blocks, no room */
    }
    return tot;
}

int sh_crf_post_ok(const_scrappie_matrix m) {
    return m && m->data.f && m->nr == 25 && m->nc >= 1 && m->stride >= 25;
}

/* Matrices trans[order[0 .. n)] (all sh_crf_post_ok) end to end into dst, each with its own stride, and the per-slot words of a launch of npad = 16
 * ntile slots (slots n .. npad - 1: no read): first float, stride, blocks; per tile its longest read.  A matrix is read as far as its last column's
 * 25th float (a caller's own container need not be padded behind it).  Returns the floats the matrices take (an even number). */
size_t sh_crf_post_stage(const const_scrappie_matrix *trans, const size_t *order, size_t n, size_t npad, float *dst,
                         long long *foff, int *stride, int *T, int *tile_T) {
    size_t at = 0;
    for (size_t t = 0; t < npad / 16; t++) tile_T[t] = 0;
    for (size_t k = 0; k < npad; k++) {
        foff[k] = 0; stride[k] = 0; T[k] = 0;
        if (k >= n) continue;
        const_scrappie_matrix m = trans[order[k]];
        if (dst) memcpy(dst + at, m->data.f, ((m->nc - 1) * m->stride + 25) * sizeof(float));
        foff[k] = (long long)at; stride[k] = (int)m->stride; T[k] = (int)m->nc;
        if (T[k] > tile_T[k / 16]) tile_T[k / 16] = T[k];
        at += m->nc * m->stride;
    }
    return (at + 1) & ~(size_t)1;
}

scrappie_matrix sh_crf_post_take(const float *src, size_t nblock) {
    scrappie_matrix post = make_scrappie_matrix(5, nblock + 1);
    if (!post) return NULL;
    for (size_t c = 0; c <= nblock; c++) memcpy(post->data.f + c * post->stride, src + c * 5, 5 * sizeof(float));
    return post;
}

/* ------------------------------------------------------------------ */
/* T4 model names (networks.c:17-34, :49-68)                            */
/* ------------------------------------------------------------------ */
static const char *const MODEL_NAMES[] = { "raw_r94", "rgrgr_r94", "rgrgr_r941", "rgrgr_r10", "rnnrf_r94" };

enum raw_model_type get_raw_model(const char *modelstr) {
    if (modelstr)
        for (int i = 0; i < 5; i++)
            if (0 == strcmp(modelstr, MODEL_NAMES[i])) return (enum raw_model_type)i;
    return SCRAPPIE_MODEL_INVALID;
}

const char *raw_model_string(const enum raw_model_type model) {
    if ((int)model < 0 || model >= SCRAPPIE_MODEL_INVALID) {
        /* the reference calls errx(EXIT_FAILURE, ...) here (networks.c:61-64) */
        fprintf(stderr, "Invalid scrappie model %s:%d\n", __FILE__, __LINE__);
        exit(EXIT_FAILURE);
    }
    return MODEL_NAMES[model];
}

/* ------------------------------------------------------------------ */
/* O1 output records (scrappie_raw.c:317-331)                           */
/* ------------------------------------------------------------------ */
int scrappie_hip_format_fasta(char *buf, size_t buflen, const char *uuid, const char *readname,
                              bool uuid_primary, const char *prefix, const scrappie_hip_call *res,
                              size_t nsample, size_t trim_start, size_t trim_end) {
    if (!uuid) uuid = "";
    return snprintf(buf, buflen,
                    ">%s%s  { \"filename\" : \"%s\", \"uuid\" : \"%s\", \"normalised_score\" : %f,  "
                    "\"nblock\" : %zu,  \"sequence_length\" : %zu,  \"blocks_per_base\" : %f, "
                    "\"nsample\" : %zu, \"trim\" : [ %zu, %zu ] }\n%s\n",
                    prefix ? prefix : "", uuid_primary ? uuid : readname, readname, uuid,
                    -res->score / res->nblock, res->nblock, res->basecall_length,
                    (float)res->nblock / (float)res->basecall_length,
                    nsample, trim_start, trim_end, res->basecall);
}

int scrappie_hip_format_sam(char *buf, size_t buflen, const char *uuid, const char *readname,
                            bool uuid_primary, const char *prefix, const scrappie_hip_call *res) {
    if (!uuid) uuid = "";
    return snprintf(buf, buflen, "%s%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*\n", prefix ? prefix : "",
                    uuid_primary ? uuid : readname, res->basecall);
}


/* ------------------------------------------------------------------ */
/* events features                                      */
/* ------------------------------------------------------------------ */
#if defined(__SSE__) || defined(__x86_64__)
#include <xmmintrin.h>
#endif

/* nanonet_features_from_events(et, true) (nnfeatures.c:51-110) followed by window(., 3, 1)
 * (layers.c:119-147).  The studentisation uses the hardware reciprocal-sqrt estimate as the
 * reference does (rsqrtps); the window leaves output column 0 zero (its loop compares an int
 * with a size_t and a negative start index ends it at once). */
int scrappie_hip_event_features(const event_table et, float *out) {
    if (!et.event || !out || et.end <= et.start) return -1;
    const size_t n = et.end - et.start;
    float *f = malloc(n * 4 * sizeof(float));
    if (!f) return -1;
    for (size_t ev = 0; ev < n; ev++) {
        const event_t *e = et.event + et.start + ev;
        f[4 * ev + 0] = e->mean;
        f[4 * ev + 1] = e->stdv;
        f[4 * ev + 2] = e->length;
        f[4 * ev + 3] = (ev + 1 < n) ? (float)fabs(e->mean - e[1].mean) : 0.0f;
    }
    float sum[4] = {0, 0, 0, 0}, sumsq[4] = {0, 0, 0, 0}, comp[4] = {0, 0, 0, 0}, compsq[4] = {0, 0, 0, 0};
    for (size_t ev = 0; ev < n; ev++)
        for (int k = 0; k < 4; k++) {
            const float x = f[4 * ev + k];
            const float d1 = x - comp[k];
            const float s1 = sum[k] + d1;
            comp[k] = (s1 - sum[k]) - d1;
            sum[k] = s1;
            const float d2 = x * x - compsq[k];
            const float s2 = sumsq[k] + d2;
            compsq[k] = (s2 - sumsq[k]) - d2;
            sumsq[k] = s2;
        }
    float scale[4], shift[4];
    for (int k = 0; k < 4; k++) {
        sum[k] /= (float)(int)n;
        sumsq[k] /= (float)(int)n;
        sumsq[k] -= sum[k] * sum[k];
    }
#if defined(__SSE__) || defined(__x86_64__)
    _mm_storeu_ps(scale, _mm_rsqrt_ps(_mm_loadu_ps(sumsq)));
#else
    for (int k = 0; k < 4; k++) scale[k] = 1.0f / sqrtf(sumsq[k]);
#endif
    for (int k = 0; k < 4; k++) shift[k] = sum[k] * scale[k];
    for (size_t ev = 0; ev < n; ev++)
        for (int k = 0; k < 4; k++) f[4 * ev + k] = scale[k] * f[4 * ev + k] - shift[k];
    memset(out, 0, n * 12 * sizeof(float));
    for (size_t col = 1; col < n; col++)                 /* column 0 stays zero */
        for (int w = 0; w < 3; w++) {
            const size_t src = col - 1 + (size_t)w;
            if (src < n) memcpy(out + col * 12 + 4 * w, f + 4 * src, 4 * sizeof(float));
        }
    free(f);
    return 0;
}

/* ------------------------------------------------------------------ */
/* block-based mapping: band checks and sequence encoding              */
/* (decode.c:1638-1689, scrappie_seq_helpers.c:30-74)                   */
/* ------------------------------------------------------------------ */
/* A band is [low[i], high[i]) per block: starts at 0, ends at seqlen, inside [0, seqlen], never empty the wrong way round,
 * monotone, and each block reaches back to the one before (low[i] == high[i-1] allowed: a step but no stay).  Every rule is
 * checked and reported (verbose) so that a caller sees all that is wrong at once, as the reference does. */
int sh_bounds_sane(const size_t *low, const size_t *high, size_t nblock, size_t seqlen, int verbose) {
#define SH_BAND_BAD(...) do { if (verbose) warnx(__VA_ARGS__); ok = 0; } while (0)
    if (!low || !high) {
        if (verbose) warnx("One or more bounds are NULL");
        return 0;
    }
    if (nblock == 0) {
        if (verbose) warnx("No blocks to bound");
        return 0;
    }
    int ok = 1;
    if (low[0] != 0) SH_BAND_BAD("First bound must include 0 (got %zu)", low[0]);
    if (high[nblock - 1] != seqlen) SH_BAND_BAD("Last bound must equal seqlen %zu (got %zu)", seqlen, high[nblock - 1]);
    for (size_t i = 0; i < nblock; i++) {
        if (low[i] > seqlen) SH_BAND_BAD("Low bound for block %zu exceeds length of sequence (got %zu but seqlen is %zu)", i, low[i], seqlen);
        if (high[i] > seqlen) SH_BAND_BAD("High bound for block %zu exceeds length of sequence (got %zu but seqlen is %zu)", i, high[i], seqlen);
        if (low[i] > high[i]) SH_BAND_BAD("Low bound for block %zu exceeds high bound [%zu , %zu).", i, low[i], high[i]);
        if (i == 0) continue;
        if (low[i] > high[i - 1])
            SH_BAND_BAD("Blocks %zu and %zu don't overlap [%zu , %zu) -> [%zu , %zu)", i - 1, i, low[i - 1], high[i - 1], low[i], high[i]);
        if (low[i] < low[i - 1])
            SH_BAND_BAD("Low bounds for blocks %zu and %zu aren't monotonic [%zu , %zu) -> [%zu , %zu)", i - 1, i, low[i - 1], high[i - 1], low[i], high[i]);
        if (high[i] < high[i - 1])
            SH_BAND_BAD("High bounds for blocks %zu and %zu aren't monotonic [%zu , %zu) -> [%zu , %zu)", i - 1, i, low[i - 1], high[i - 1], low[i], high[i]);
    }
#undef SH_BAND_BAD
    return ok;
}

bool are_bounds_sane(size_t const *low, size_t const *high, size_t nblock, size_t seqlen) {
    return sh_bounds_sane(low, high, nblock, seqlen, 1) != 0;
}

/* The loop the four pack planners below share: member k of len[k] + per cells, in input order, into packs that open with `open` cells and hold
 * at most pack_cells (at most maxc whatever is asked for); -1 entries where a member fits no pack or, with `empty`, has no length. */
static long pack_plan(const size_t *len, size_t n, size_t pack_cells, size_t maxc, size_t per, size_t open, int empty, int *pack, long long *cell) {
    if (!len || !pack || !cell) return 0;
    if (pack_cells > maxc) pack_cells = maxc;
    long np = 0;
    size_t used = 0;                    /* cells of the open pack, np - 1; 0: none is open */
    for (size_t k = 0; k < n; k++) {
        if ((empty && len[k] == 0) || len[k] > maxc - per - open) { pack[k] = -1; cell[k] = -1; continue; }
        const size_t c = len[k] + per;
        if (used == 0 || used + c > pack_cells) { np++; used = open; }
        pack[k] = (int)(np - 1);
        cell[k] = (long long)used;
        used += c;
    }
    return np;
}

/* Packs of candidates (k_map_pack, sh_map_pack.h): a candidate of L states takes L + 2 cells, a pack of ncell cells and ncand
 * candidates two rows of floats, a word per cell and ncand + 1 first cells in LDS. */
size_t sh_map_pack_lds_bytes(size_t ncell, size_t ncand) { return (3 * ncell + ncand + 1) * 4; }

/* the most cells a pack may hold: what fits SH_MAP_LDS however the cells are shared out among candidates -- a candidate has at least
 * 3 cells, so ncell cells hold ncell / 3 candidates at most, and the bytes only grow with ncell */
size_t scrappie_hip_map_pack_max_cells(void) {
    size_t c = SH_MAP_LDS / 12;
    while (c > 0 && sh_map_pack_lds_bytes(c, c / 3) > SH_MAP_LDS) c--;
    return c;
}

/* Candidates of seqlen[k] states into packs of at most pack_cells cells (at most scrappie_hip_map_pack_max_cells() whatever is
 * asked for), in input order: a pack is closed when the next candidate would take it past pack_cells, so a candidate of more
 * cells than that is alone in its pack.  pack[k]: the candidate's pack, cell[k]: its first cell there; pack[k] = -1 (cell[k] = -1)
 * where its seqlen[k] + 2 cells exceed the most a pack may hold -- such a candidate takes k_map.  Returns the number of packs. */
long scrappie_hip_map_pack_plan(const size_t *seqlen, size_t ncand, size_t pack_cells, int *pack, long long *cell) {
    return pack_plan(seqlen, ncand, pack_cells, scrappie_hip_map_pack_max_cells(), 2, 0, 0, pack, cell);
}

/* Packs of candidate squiggles (k_squig_pack, sh_squig_pack.h; the word counts and the cell words: sh_internal.h). */
size_t sh_squig_pack_lds_bytes(size_t ncell, size_t ncand, size_t npiece) {
    return (SH_SQP_CELL_WORDS * ncell + SH_SQP_CAND_WORDS * ncand + SH_SQP_PIECE_WORDS * npiece) * 4;
}

/* the most cells a pack may hold: what fits SH_SQ_LDS however the cells are shared out among candidates -- a candidate has at least
 * one cell and a piece at least one, so ncell cells are ncell candidates and ncell pieces at most, and the bytes only grow with ncell */
size_t scrappie_hip_squiggle_pack_max_cells(void) {
    size_t c = SH_SQ_LDS / (SH_SQP_CELL_WORDS * 4);
    while (c > 0 && sh_squig_pack_lds_bytes(c, c, c) > SH_SQ_LDS) c--;
    return c <= SH_SQP_POS_MASK ? c : SH_SQP_POS_MASK;      /* (what a cell word's fields hold) */
}

/* Candidates of npos[k] positions (a cell each) into packs of at most pack_cells cells (at most scrappie_hip_squiggle_pack_max_cells()
 * whatever is asked for), in input order: a pack is closed when the next candidate would take it past pack_cells, so a candidate of
 * more cells than that is alone in its pack.  pack[k]: the candidate's pack, cell[k]: its first cell there; pack[k] = -1
 * (cell[k] = -1) where npos[k] exceeds the most a pack may hold -- such a candidate takes k_squig -- or is 0.  Returns the number of
 * packs. */
long scrappie_hip_squiggle_pack_plan(const size_t *npos, size_t ncand, size_t pack_cells, int *pack, long long *cell) {
    return pack_plan(npos, ncand, pack_cells, scrappie_hip_squiggle_pack_max_cells(), 0, 0, 1, pack, cell);
}

size_t sh_squig_pack_layout(const size_t *npos, size_t ncand, int *wa, int *wb, int *piece0, int *npiece) {
    size_t g = 0, piece = 0;
    for (size_t k = 0; k < ncand; k++) {
        const size_t n = npos[k];
        if (piece0) piece0[k] = (int)piece;
        for (size_t pos = 0; pos < n; pos++, g++) {
            const int head = pos == 0 || g % 64 == 0;
            if (head && pos) piece++;
            if (wa) wa[g] = (int)pos | (int)(k << SH_SQP_CAND_SHIFT) | (pos == 0 ? SH_SQP_POS0 : 0) | (pos == 1 ? SH_SQP_POS1 : 0) | (pos + 2 <= n ? SH_SQP_RIGHT : 0);
            if (wb) wb[g] = (int)piece | (head ? SH_SQP_HEAD : 0);
        }
        if (n) piece++;
        if (npiece) npiece[k] = (int)piece - (piece0 ? piece0[k] : 0);
    }
    return piece;
}

/* The same for the tests, from the plan above: the candidates k with pack[k] == which, in their order, laid out as their pack holds
 * them.  wa / wb: the pack's cell words, piece0 / npiece: per candidate OF THE CALL (untouched for those of other packs); returns the
 * pack's pieces (0 too where memory runs out). */
size_t scrappie_hip_squiggle_pack_layout(const size_t *npos, size_t ncand, const int *pack, int which, int *wa, int *wb, int *piece0, int *npiece) {
    if (!npos || !pack) return 0;
    size_t n = 0;
    for (size_t k = 0; k < ncand; k++) n += pack[k] == which;
    if (n == 0) return 0;
    size_t *len = malloc(n * sizeof(size_t));
    int *p0 = malloc(2 * n * sizeof(int));
    size_t np = 0;
    if (len && p0) {
        size_t j = 0;
        for (size_t k = 0; k < ncand; k++) if (pack[k] == which) len[j++] = npos[k];
        np = sh_squig_pack_layout(len, n, wa, wb, p0, p0 + n);
        j = 0;
        for (size_t k = 0; k < ncand; k++) {
            if (pack[k] != which) continue;
            if (piece0) piece0[k] = p0[j];
            if (npiece) npiece[k] = p0[n + j];
            j++;
        }
    }
    free(len); free(p0);
    return np;
}

/* Bands of the CRF mapping (k_map_crf, sh_map_crf.h): per ENTRY t = 0 .. nblock of the path (nblock + 1 of them) the cells
 * [low[t], high[t]) of 0 .. seqlen, a cell being the number of bases emitted so far.  Valid: it starts at cell 0 and ends with
 * cell seqlen, is never empty or beyond seqlen + 1, both edges non-decreasing, and every entry's lowest cell has a predecessor
 * (itself or the cell below) in the entry before.  Quiet: 1 / 0. */
int scrappie_hip_map_crf_bounds_sane(const size_t *low, const size_t *high, size_t nblock, size_t seqlen) {
    if (!low || !high || nblock == 0 || seqlen == 0) return 0;
    if (low[0] != 0 || high[nblock] != seqlen + 1) return 0;
    for (size_t t = 0; t <= nblock; t++) {
        if (low[t] >= high[t] || high[t] > seqlen + 1) return 0;
        if (t == 0) continue;
        if (low[t] < low[t - 1] || high[t] < high[t - 1] || low[t] > high[t - 1]) return 0;
    }
    return 1;
}

/* the diagonal through (entry 0, cell 0) and (entry nblock, cell seqlen), halfwidth cells to either side, clamped into
 * 0 .. seqlen and, where the diagonal is steeper than the band is wide, reaching back to the entry before: always a band that
 * scrappie_hip_map_crf_bounds_sane accepts.  low, high: nblock + 1 entries each.  0, or -1 on a null or empty argument. */
int scrappie_hip_map_crf_diagonal_band(size_t nblock, size_t seqlen, size_t halfwidth, size_t *low, size_t *high) {
    if (!low || !high || nblock == 0 || seqlen == 0) return -1;
    for (size_t t = 0; t <= nblock; t++) {
        const size_t c = (size_t)(((unsigned long long)t * (unsigned long long)seqlen) / (unsigned long long)nblock);
        low[t] = c > halfwidth ? c - halfwidth : 0;
        high[t] = (halfwidth >= seqlen || c + halfwidth + 1 > seqlen + 1) ? seqlen + 1 : c + halfwidth + 1;
        if (t > 0 && low[t] > high[t - 1]) low[t] = high[t - 1];
    }
    return 0;
}

/* The cut of a reference into windows that the three reference-local planners below share.  Of `cells` cells window w owns the s entry
 * cells from w s on and holds reach cells more, where a path that enters it can get to -- and, back: one cell to the left of its own where
 * it is not the first --, as far as there are cells: first[w], own[w], ncell[w].  home[w]: 0 rows in LDS, 1 (more than maxc cells) rows in
 * device scratch, at float offset scr_off[w] (-1 in LDS) of *scr_floats floats in all, scr(ncell) per window.  Every array may be NULL;
 * those given hold cap entries, and only the first cap windows are written.  Returns the number of windows. */
static long long win_plan(size_t cells, size_t s, size_t reach, int back, size_t maxc, size_t (*scr_of)(size_t), size_t cap, size_t *first, size_t *ncell,
                          size_t *own, int *home, long long *scr_off, long long *scr_floats) {
    const size_t nwin = (cells + s - 1) / s;
    long long scr = 0;
    for (size_t w = 0; w < nwin; w++) {
        const size_t p0 = w * s;                                /* the first entry cell it owns */
        const size_t c0 = back && p0 ? p0 - 1 : p0;
        const size_t left = cells - p0;                         /* cells from p0 to the end */
        const size_t nc = (s + reach < left ? p0 + s + reach : cells) - c0;
        const int scratch = nc > maxc;
        if (w < cap) {
            if (first) first[w] = c0;
            if (ncell) ncell[w] = nc;
            if (own) own[w] = s < left ? s : left;
            if (home) home[w] = scratch;
            if (scr_off) scr_off[w] = scratch ? scr : -1;
        }
        if (scratch) scr += (long long)scr_of(nc);
    }
    if (scr_floats) *scr_floats = scr;
    return (long long)nwin;
}

/* Windows of the sequence-local CRF mapping (k_map_crf_local, sh_map_crf_local.h).  A window of ncell cells keeps two columns of
 * transitions, four rows of ncell + 1 floats and ncell codes in LDS. */
size_t sh_map_crf_local_lds_bytes(size_t ncell) { return (64 + 4 * (ncell + 1) + ncell) * 4; }
static size_t map_crf_local_scr_floats(size_t ncell) { return 4 * (ncell + 1); }      /* the four rows of a window in device scratch */

/* the most cells a window keeps in LDS (the bytes are linear in ncell) */
size_t scrappie_hip_map_crf_local_max_cells(void) {
    const size_t per = sh_map_crf_local_lds_bytes(1) - sh_map_crf_local_lds_bytes(0);
    return (SH_MAP_LDS - sh_map_crf_local_lds_bytes(0)) / per;
}

/* The stride in cells a sequence of seqlen bases and a read of nblock blocks are cut with.  stride > 0: that many cells; 0: one
 * window; < 0: the default -- a window (stride + nblock cells) of SH_MAP_CRF_LOCAL_CELLS cells, of which four are resident per
 * compute unit, while the window owns at least half of its cells (stride >= nblock); the largest stride whose window is
 * LDS-resident beyond; and nblock, with the rows in device scratch, where nblock + 1 cells alone exceed the LDS home
 * (profiles/map_crf_local_rate.txt decided between them).  Never more than the seqlen + 1 cells there are. */
size_t scrappie_hip_map_crf_local_stride(size_t seqlen, size_t nblock, long stride) {
    const size_t cells = seqlen + 1, maxc = scrappie_hip_map_crf_local_max_cells();
    size_t s;
    if (stride > 0) s = (size_t)stride;
    else if (stride == 0) s = cells;
    else if (nblock + 1 > maxc) s = nblock;
    else if (2 * nblock <= SH_MAP_CRF_LOCAL_CELLS && SH_MAP_CRF_LOCAL_CELLS <= maxc) s = SH_MAP_CRF_LOCAL_CELLS - nblock;
    else s = maxc - nblock;
    if (s == 0) s = 1;
    return s < cells ? s : cells;
}

/* The cut: window w owns the start cells [w s, min((w + 1) s, seqlen + 1)) and holds the cells [w s, min(w s + s - 1 + nblock,
 * seqlen)] -- first[w], own[w] and ncell[w]; home[w]: 0 rows and codes in LDS, 1 rows in device scratch, at float offset
 * scr_off[w] (-1 in LDS) of *scr_floats floats in all, 4 (ncell + 1) per window: whole 16-byte pieces.  Every array may be NULL;
 * those given hold cap entries, and only the first cap windows are written.  Returns the number of windows, 0 on an empty
 * sequence, no blocks or a sequence beyond 2^30 bases (a cell and its kind share an int32). */
long long scrappie_hip_map_crf_local_plan(size_t seqlen, size_t nblock, long stride, size_t cap, size_t *first, size_t *ncell, size_t *own,
                                          int *home, long long *scr_off, long long *scr_floats) {
    if (scr_floats) *scr_floats = 0;
    if (seqlen == 0 || nblock == 0 || seqlen > ((size_t)1 << 30) || nblock > ((size_t)1 << 30)) return 0;
    return win_plan(seqlen + 1, scrappie_hip_map_crf_local_stride(seqlen, nblock, stride), nblock, 0, scrappie_hip_map_crf_local_max_cells(),
                    map_crf_local_scr_floats, cap, first, ncell, own, home, scr_off, scr_floats);
}

/* Windows of the sequence-local transducer mapping (k_map_local, sh_map_local.h).  A window keeps a head of 32 words and two
 * columns of the posterior (nr states, rounded up to whole 16-byte pieces) in LDS; in the LDS home also two score rows, the END
 * row and the codes, each of ncell entries rounded up to a multiple of 4. */
size_t sh_map_local_scr_lds_bytes(size_t nr) { return (32 + 2 * ((nr + 3) & ~(size_t)3)) * 4; }
size_t sh_map_local_lds_bytes(size_t ncell, size_t nr) { return sh_map_local_scr_lds_bytes(nr) + 4 * ((ncell + 3) & ~(size_t)3) * 4; }
static size_t map_local_scr_floats(size_t ncell) { return 3 * ((ncell + 3) & ~(size_t)3); }      /* the three rows of a window in device scratch */

/* the most cells a window of a posterior of nr states keeps in LDS; 0 where the columns alone exceed it */
size_t scrappie_hip_map_local_max_cells(size_t nr) {
    const size_t fixed = sh_map_local_scr_lds_bytes(nr);
    return fixed >= SH_MAP_LDS ? 0 : ((SH_MAP_LDS - fixed) / 16) & ~(size_t)3;      /* (a row is a multiple of 4 entries) */
}

/* The stride in positions a sequence of seqlen states and a read of nblock blocks are cut with.  A path that enters at a position
 * advances at most reach = 2 (nblock - 1) positions, so a window is stride + reach cells.  stride > 0: that many; 0: one window;
 * < 0: the default -- while a window that owns more than half of its cells (stride >= reach + 1) fits LDS: a window of
 * SH_MAP_LOCAL_CELLS cells where that leaves it the SH_MAP_LOCAL_STRIDE entry positions it was measured with or more
 * (profiles/map_local_rate.txt decided), the largest LDS-resident window for longer reads; and 2 nblock, with the rows in device
 * scratch, beyond.  Never more than the seqlen positions there are. */
size_t scrappie_hip_map_local_stride(size_t seqlen, size_t nblock, size_t nr, long stride) {
    const size_t maxc = scrappie_hip_map_local_max_cells(nr), reach = nblock ? 2 * (nblock - 1) : 0;
    size_t s;
    if (stride > 0) s = (size_t)stride;
    else if (stride == 0) s = seqlen;
    else if (2 * reach + 1 > maxc) s = 2 * nblock;
    else if (reach + SH_MAP_LOCAL_STRIDE <= SH_MAP_LOCAL_CELLS && SH_MAP_LOCAL_CELLS <= maxc) s = SH_MAP_LOCAL_CELLS - reach;
    else s = maxc - reach;
    if (s == 0) s = 1;
    return s < seqlen ? s : seqlen;
}

/* The cut: window w owns the entry positions [w s, min((w + 1) s, seqlen)) and holds the cells [w s, min(w s + s - 1 + 2 (nblock - 1),
 * seqlen - 1)] -- first[w], own[w] and ncell[w]; home[w]: 0 rows and codes in LDS, 1 rows in device scratch, at float offset
 * scr_off[w] (-1 in LDS) of *scr_floats floats in all, 3 * 4 ceil(ncell / 4) per window: whole 16-byte pieces.  Every array may be
 * NULL; those given hold cap entries, and only the first cap windows are written.  Returns the number of windows, 0 on an empty
 * sequence, no blocks, fewer than 2 states or a sequence or read beyond 2^30. */
long long scrappie_hip_map_local_plan(size_t seqlen, size_t nblock, size_t nr, long stride, size_t cap, size_t *first, size_t *ncell, size_t *own,
                                      int *home, long long *scr_off, long long *scr_floats) {
    if (scr_floats) *scr_floats = 0;
    if (seqlen == 0 || nblock == 0 || nr < 2 || seqlen > ((size_t)1 << 30) || nblock > ((size_t)1 << 30)) return 0;
    return win_plan(seqlen, scrappie_hip_map_local_stride(seqlen, nblock, nr, stride), 2 * (nblock - 1), 0, scrappie_hip_map_local_max_cells(nr),
                    map_local_scr_floats, cap, first, ncell, own, home, scr_off, scr_floats);
}

/* Windows of the reference-local squiggle mapping (k_squig_local, sh_squig_local.h).  In the LDS home a window of ncell cells keeps
 * a head of 16 words, two rows of a position and a back value per cell, the END row, and its slice of the tables: loc, scale, logsc
 * and stay per cell and ncell + 2 move entries -- 10 words per cell and 18 beside them.  In the scratch home only the head. */
size_t sh_squig_local_scr_lds_bytes(void) { return 16 * 4; }
size_t sh_squig_local_lds_bytes(size_t ncell) { return (16 + 10 * ncell + 2) * 4; }
/* the five rows of a window in device scratch, whole 16-byte pieces */
size_t sh_squig_local_scr_floats(size_t ncell) { return (5 * ncell + 3) & ~(size_t)3; }

/* the most cells a window keeps in LDS (the bytes are linear in ncell) */
size_t scrappie_hip_squiggle_local_max_cells(void) {
    const size_t per = sh_squig_local_lds_bytes(1) - sh_squig_local_lds_bytes(0);
    return (SH_SQ_LDS - sh_squig_local_lds_bytes(0)) / per;
}

/* The stride in positions a reference of npos positions and a read of nsample samples are cut with.  A path that enters at a
 * position advances at most 2 (nsample - 1) positions and reaches one cell to the left, so a window is stride + 2 (nsample - 1) + 1
 * cells.  stride > 0: that many; 0: one window; < 0: the default -- the largest LDS-resident window while it owns at least half of
 * its cells; SH_SQUIG_LOCAL_SCR_MUL nsample, with the rows in device scratch, beyond (profiles/squiggle_local_rate.txt decided).
 * Never more than the npos positions there are. */
size_t scrappie_hip_squiggle_local_stride(size_t npos, size_t nsample, long stride) {
    const size_t maxc = scrappie_hip_squiggle_local_max_cells(), reach = nsample ? 2 * (nsample - 1) + 1 : 1;
    size_t s;
    if (stride > 0) s = (size_t)stride;
    else if (stride == 0) s = npos;
    else if (2 * reach <= maxc) s = maxc - reach;
    else s = SH_SQUIG_LOCAL_SCR_MUL * nsample;
    if (s == 0) s = 1;
    return s < npos ? s : npos;
}

/* The cut: window w owns the entry positions [w s, min((w + 1) s, npos)) -- own[w] of them -- and holds the cells [max(w s - 1, 0),
 * min(w s + s - 1 + 2 (nsample - 1), npos - 1)] -- first[w] and ncell[w]; home[w]: 0 rows and tables in LDS, 1 rows in device
 * scratch, at float offset scr_off[w] (-1 in LDS) of *scr_floats floats in all, 5 ncell per window rounded up to whole 16-byte
 * pieces.  Every array may be NULL; those given hold cap entries, and only the first cap windows are written.  Returns the number of
 * windows, 0 on an empty reference, no samples or either beyond 2^30. */
long long scrappie_hip_squiggle_local_plan(size_t npos, size_t nsample, long stride, size_t cap, size_t *first, size_t *ncell, size_t *own,
                                           int *home, long long *scr_off, long long *scr_floats) {
    if (scr_floats) *scr_floats = 0;
    if (npos == 0 || nsample == 0 || npos > ((size_t)1 << 30) || nsample > ((size_t)1 << 30)) return 0;
    return win_plan(npos, scrappie_hip_squiggle_local_stride(npos, nsample, stride), 2 * (nsample - 1), 1 /* back state p0 - 1 lives in the cell to its left */,
                    scrappie_hip_squiggle_local_max_cells(), sh_squig_local_scr_floats, cap, first, ncell, own, home, scr_off, scr_floats);
}

/* Packs of motifs searched inside a flip-flop read (k_crf_find, sh_crf_find.h).  A pack of ncell cells keeps two columns of
 * transitions and, per cell and the spare slot behind them, two buffers of a value and a stay value (16 bytes) and a word (4);
 * with positions two buffers of two payloads more (16): 20 or 36 bytes per cell. */
size_t sh_crf_find_lds_bytes(size_t ncell, int pos) { return (64 + (pos ? 9 : 5) * (ncell + 1)) * 4; }

/* the most cells a pack may hold, the read's five U cells included: what the LDS holds with positions (the bytes are linear in ncell) */
size_t scrappie_hip_crf_find_max_cells(void) {
    const size_t per = sh_crf_find_lds_bytes(1, 1) - sh_crf_find_lds_bytes(0, 1);
    return (SH_MAP_LDS - sh_crf_find_lds_bytes(0, 1)) / per;
}

/* Motifs of seqlen[k] bases into packs of at most pack_cells cells (at most scrappie_hip_crf_find_max_cells() whatever is asked
 * for), in input order.  A pack begins with the read's five U cells; a motif of L bases takes L - 1 interior cells and five V
 * cells behind them.  A pack is closed when the next motif would take it past pack_cells, so a motif of more cells than that is
 * alone in its pack.  pack[k]: the motif's pack, cell[k]: its first cell there (5 for the first); pack[k] = -1 (cell[k] = -1) for
 * an empty motif and where 5 + seqlen[k] + 4 cells exceed the most a pack may hold -- such a motif is not mapped.  Returns the
 * number of packs. */
long scrappie_hip_crf_find_plan(const size_t *seqlen, size_t nmotif, size_t pack_cells, int *pack, long long *cell) {
    return pack_plan(seqlen, nmotif, pack_cells, scrappie_hip_crf_find_max_cells(), 4, 5, 1, pack, cell);
}

/* Packs of candidates a flip-flop read is mapped to (k_map_crf_pack, sh_map_crf_pack.h).  A pack of ncell cells keeps two columns of
 * transitions (64 floats) and, per cell and the spare slot behind them, two buffers of a B and an S value (16 bytes) and a word (4). */
size_t sh_map_crf_pack_lds_bytes(size_t ncell) { return (64 + 5 * (ncell + 1)) * 4; }

/* the most cells a pack may hold: what SH_MAP_LDS holds (the bytes are linear in ncell) */
size_t scrappie_hip_map_crf_pack_max_cells(void) {
    const size_t per = sh_map_crf_pack_lds_bytes(1) - sh_map_crf_pack_lds_bytes(0);
    return (SH_MAP_LDS - sh_map_crf_pack_lds_bytes(0)) / per;
}

/* Candidates of seqlen[k] bases into packs of at most pack_cells cells (at most scrappie_hip_map_crf_pack_max_cells() whatever is
 * asked for), in input order: a candidate of L bases takes L + 1 cells; a pack is closed when the next candidate would take it past
 * pack_cells, so a candidate of more cells than that is alone in its pack.  pack[k]: the candidate's pack, cell[k]: its first cell
 * there; pack[k] = -1 (cell[k] = -1) where its seqlen[k] + 1 cells exceed the most a pack may hold -- such a candidate takes
 * k_map_crf, and does not close the open pack.  Returns the number of packs. */
long scrappie_hip_map_crf_pack_plan(const size_t *seqlen, size_t ncand, size_t pack_cells, int *pack, long long *cell) {
    return pack_plan(seqlen, ncand, pack_cells, scrappie_hip_map_crf_pack_max_cells(), 1, 0, 0, pack, cell);
}

/* Every single-base edit of a sequence against a flip-flop read (k_crf_edits_rows, k_crf_edits, sh_crf_edits.h): what a read of L
 * bases and nblock blocks keeps in device memory.  Three row matrices -- F_B, F_S, G_B -- of nblock + 1 entries, an entry's row of
 * `pitch` floats: cells 0 .. L and the slot at L + 1 that takes the stores of threads without a cell, rounded up to 16 floats, so
 * every row starts on 64 bytes.  Results: sub [L][4], ins [L + 1][4], del [L], 9 L + 4 floats rounded up to 4. */
size_t scrappie_hip_crf_edits_pitch(size_t seqlen) { return (seqlen + 2 + 15) / 16 * 16; }
static size_t crf_edits_res_floats(size_t seqlen) { return (9 * seqlen + 4 + 3) / 4 * 4; }
size_t scrappie_hip_crf_edits_row_bytes(size_t seqlen, size_t nblock) { return 3 * (nblock + 1) * scrappie_hip_crf_edits_pitch(seqlen) * 4; }

/* The pitch of a read in a band of `entries` entries: an entry's row holds its band's cells alone and a last slot that is no cell's; one pitch per
 * read, the widest entry's cells and that slot rounded up to 16 floats.  An entry that is empty or the wrong way round counts as one cell (the
 * engines refuse such a band before they plan).  0: a null argument. */
static size_t edits_band_pitch(const size_t *low, const size_t *high, size_t entries) {
    size_t w = 1;
    if (!low || !high) return 0;
    for (size_t t = 0; t < entries; t++)
        if (high[t] > low[t] && high[t] - low[t] > w) w = high[t] - low[t];
    return (w + 1 + 15) / 16 * 16;
}

/* The layout that the four planners of the edit engines below share, k 0 for the flip-flop family (three row matrices, bands of nblock + 1
 * entries; else two, of nblock): read i takes its family's pitch -- where low and high are given and neither of low[i], high[i] is NULL, its
 * band's -- and nblock[i] + 1 rows of it per matrix; the reads lie one behind the other in input order in the row buffer and in the result
 * buffer.  Returns the floats of the row buffer; *res_floats (may be NULL): those of the result buffer. */
static long long edits_plan(const size_t *seqlen, const size_t *nblock, const size_t *const *low, const size_t *const *high, size_t n, size_t k, int *pitch,
                            long long *rows, long long *res, long long *res_floats) {
    long long nrow = 0, nres = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t p = low && high && low[i] && high[i] ? edits_band_pitch(low[i], high[i], k ? nblock[i] : nblock[i] + 1)
                         : k ? scrappie_hip_map_edits_pitch(seqlen[i], k) : scrappie_hip_crf_edits_pitch(seqlen[i]);
        pitch[i] = (int)p;
        rows[i] = nrow;
        res[i] = nres;
        nrow += (long long)((k ? 2 : 3) * (nblock[i] + 1) * p);
        nres += (long long)crf_edits_res_floats(seqlen[i]);
    }
    if (res_floats) *res_floats = nres;
    return nrow;
}

/* Reads of seqlen[i] bases and nblock[i] blocks in one launch, in input order: pitch[i], rows[i] -- the float offset of read i's F_B
 * in the launch's row buffer; F_S lies (nblock[i] + 1) * pitch[i] floats behind it and G_B as many behind F_S -- and res[i], the
 * float offset of its results in the result buffer.  Both offsets are multiples of 4 floats (16 bytes); no two reads overlap.
 * Returns the floats of the row buffer; *res_floats (may be NULL): those of the result buffer. */
long long scrappie_hip_crf_edits_plan(const size_t *seqlen, const size_t *nblock, size_t n, int *pitch, long long *rows, long long *res,
                                      long long *res_floats) {
    if (res_floats) *res_floats = 0;
    if (!seqlen || !nblock || !pitch || !rows || !res) return 0;
    return edits_plan(seqlen, nblock, NULL, NULL, n, 0, pitch, rows, res, res_floats);
}

/* The same in a band (low, high: nblock + 1 entries each, as scrappie_hip_map_crf_bounds_sane takes them): an entry's row holds its band's
 * cells alone, cell p of entry t at float p - low[t], and the row's last slot takes the stores of threads without a cell (edits_band_pitch). */
size_t scrappie_hip_crf_edits_band_pitch(const size_t *low, const size_t *high, size_t nblock) { return edits_band_pitch(low, high, nblock + 1); }
size_t scrappie_hip_crf_edits_band_row_bytes(const size_t *low, const size_t *high, size_t nblock) {
    return 3 * (nblock + 1) * scrappie_hip_crf_edits_band_pitch(low, high, nblock) * 4;
}

/* scrappie_hip_crf_edits_plan for reads in bands: read i has the band low[i], high[i] (nblock[i] + 1 entries each); where either is NULL the read
 * has no band and takes the unbanded pitch and rows.  Everything else as there. */
long long scrappie_hip_crf_edits_band_plan(const size_t *seqlen, const size_t *nblock, const size_t *const *low, const size_t *const *high, size_t n,
                                           int *pitch, long long *rows, long long *res, long long *res_floats) {
    if (res_floats) *res_floats = 0;
    if (!seqlen || !nblock || !low || !high || !pitch || !rows || !res) return 0;
    return edits_plan(seqlen, nblock, low, high, n, 0, pitch, rows, res, res_floats);
}

/* The band around a Viterbi path of k_map_crf: path[t], t = 0 .. nblock, the index of the last base emitted through entry t (-1: none), so
 * cnt = path[t] + 1 is the path's cell; low[t] = max(cnt - halfwidth, 0), high[t] = min(cnt + halfwidth + 1, seqlen + 1), and low[0] = 0
 * whatever the half-width (a path whose entry 0 is a base is in cell 1 there; a band begins at cell 0).  A path moves by 0 or 1 per entry,
 * begins in cell 0 or 1 and ends in cell seqlen, so both edges are non-decreasing, high[nblock] = seqlen + 1 and
 * low[t] <= cnt[t - 1] + 1 - halfwidth <= high[t - 1]: always a band that scrappie_hip_map_crf_bounds_sane accepts.  -1 on a null or empty
 * argument or what is no path of that sequence: a value outside -1 .. seqlen - 1 (entry 0: outside -1 .. 0), a step down or above 1,
 * path[nblock] != seqlen - 1. */
int scrappie_hip_map_crf_path_band(const int *path, size_t nblock, size_t seqlen, size_t halfwidth, size_t *low, size_t *high) {
    if (!path || !low || !high || nblock == 0 || seqlen == 0) return -1;
    for (size_t t = 0; t <= nblock; t++) {
        if (path[t] < -1 || (long long)path[t] > (long long)seqlen - 1) return -1;
        if (t > 0 && (path[t] < path[t - 1] || path[t] - path[t - 1] > 1)) return -1;
    }
    if (path[0] > 0 || (size_t)(path[nblock] + 1) != seqlen) return -1;
    for (size_t t = 0; t <= nblock; t++) {
        const size_t cnt = (size_t)(path[t] + 1);
        low[t] = (t > 0 && cnt > halfwidth) ? cnt - halfwidth : 0;
        high[t] = (halfwidth >= seqlen || cnt + halfwidth + 1 > seqlen + 1) ? seqlen + 1 : cnt + halfwidth + 1;
    }
    return 0;
}

/* Every single-base edit of a sequence against a transducer read (k_map_edits_rows, k_map_edits, sh_map_edits.h): what a read of L
 * bases -- n = L - k + 1 states -- and nblock blocks keeps in device memory.  Two row matrices, F and G, of nblock + 1 entries, an
 * entry's row of `pitch` floats: cells 0 .. n - 1 and slot n (FS going forward, the stores of threads without a cell going backward),
 * rounded up to 16 floats, so every row starts on 64 bytes.  Results: sub [L][4], ins [L + 1][4], del [L], 9 L + 4 floats rounded up
 * to 4.  Fewer than k bases hold no state: pitch and row_bytes 0, and the plan refuses. */
size_t scrappie_hip_map_edits_pitch(size_t seqlen_bases, size_t k) {
    return (k == 0 || seqlen_bases < k) ? 0 : (seqlen_bases - k + 1 + 1 + 15) / 16 * 16;
}
size_t scrappie_hip_map_edits_row_bytes(size_t seqlen_bases, size_t k, size_t nblock) {
    return 2 * (nblock + 1) * scrappie_hip_map_edits_pitch(seqlen_bases, k) * 4;
}
/* the longest sequence in bases: its states and two rows stay in LDS as k_map's do (12 n + 16 bytes) */
size_t scrappie_hip_map_edits_max_bases(size_t k) { return k == 0 ? 0 : (SH_MAP_LDS - 16) / 12 + k - 1; }

/* Reads of seqlen[i] bases and nblock[i] blocks in one launch, in input order: pitch[i], rows[i] -- the float offset of read i's F in
 * the launch's row buffer; G lies (nblock[i] + 1) * pitch[i] floats behind it -- and res[i], the float offset of its results in the
 * result buffer.  Both offsets are multiples of 4 floats (16 bytes); no two reads overlap.  Returns the floats of the row buffer;
 * *res_floats (may be NULL): those of the result buffer.  -1: k is 0 or a read has fewer than k bases. */
long long scrappie_hip_map_edits_plan(const size_t *seqlen, const size_t *nblock, size_t n, size_t k, int *pitch, long long *rows, long long *res,
                                      long long *res_floats) {
    if (res_floats) *res_floats = 0;
    if (!seqlen || !nblock || !pitch || !rows || !res) return 0;
    if (k == 0) return -1;
    for (size_t i = 0; i < n; i++)
        if (seqlen[i] < k) return -1;
    return edits_plan(seqlen, nblock, NULL, NULL, n, k, pitch, rows, res, res_floats);
}

/* The same in a band (low, high: nblock entries each, as are_bounds_sane takes them; cell q of entry t + 1 admissible iff low[t] <= q < high[t]):
 * an entry's row holds its band's cells alone, cell q of entry t + 1 at float q - low[t], and the row's last slot holds FS (forward) or takes the
 * stores of threads without a cell (backward) (edits_band_pitch).  0: a null argument. */
size_t scrappie_hip_map_edits_band_pitch(const size_t *low, const size_t *high, size_t nblock) { return edits_band_pitch(low, high, nblock); }
size_t scrappie_hip_map_edits_band_row_bytes(const size_t *low, const size_t *high, size_t nblock) {
    return 2 * (nblock + 1) * scrappie_hip_map_edits_band_pitch(low, high, nblock) * 4;
}

/* scrappie_hip_map_edits_plan for reads in bands: read i has the band low[i], high[i] (nblock[i] entries each); where either is NULL the read has
 * no band and takes the unbanded pitch and rows.  Everything else as there. */
long long scrappie_hip_map_edits_band_plan(const size_t *seqlen, const size_t *nblock, const size_t *const *low, const size_t *const *high, size_t n,
                                           size_t k, int *pitch, long long *rows, long long *res, long long *res_floats) {
    if (res_floats) *res_floats = 0;
    if (!seqlen || !nblock || !low || !high || !pitch || !rows || !res) return 0;
    if (k == 0) return -1;
    for (size_t i = 0; i < n; i++)
        if (seqlen[i] < k) return -1;
    return edits_plan(seqlen, nblock, low, high, n, k, pitch, rows, res, res_floats);
}

/* The band around a Viterbi path of k_map: path[t], t = 0 .. nblock - 1, the state after block t (0 .. nstate - 1; -1 in START and in END).  p[t] is
 * the path's position: 0 over the leading START entries, nstate - 1 over the trailing END entries; low[t] = max(p - halfwidth, 0), high[t] =
 * min(p + halfwidth + 1, nstate), and low[0] = 0, high[nblock - 1] = nstate whatever the path.  A path moves by 0, 1 or 2 states per block, so with
 * halfwidth >= 1 low[t] <= p[t - 1] + 2 - halfwidth <= high[t - 1] and both edges are non-decreasing: always a band that are_bounds_sane accepts,
 * and the path is inside it.  -1: a null or empty argument, halfwidth < 1 (a skip moves two states: a half-width of 0 cannot hold it), or what is
 * no path of such a sequence -- a value outside -1 .. nstate - 1, a step down or above 2, a -1 between positions, no position at all, a first
 * position other than 0 (START enters state 0 alone), a last other than nstate - 1. */
int scrappie_hip_map_path_band(const int *path, size_t nblock, size_t nstate, size_t halfwidth, size_t *low, size_t *high) {
    if (!path || !low || !high || nblock == 0 || nstate == 0 || halfwidth < 1) return -1;
    size_t first = nblock, last = 0;
    for (size_t t = 0; t < nblock; t++) {
        if (path[t] < -1 || (long long)path[t] > (long long)nstate - 1) return -1;
        if (path[t] >= 0) { if (first == nblock) first = t; last = t; }
    }
    if (first == nblock || path[first] != 0 || (size_t)path[last] != nstate - 1) return -1;
    for (size_t t = first; t <= last; t++) {
        if (path[t] < 0) return -1;
        if (t > first && (path[t] < path[t - 1] || path[t] - path[t - 1] > 2)) return -1;
    }
    for (size_t t = 0; t < nblock; t++) {
        const size_t p = t < first ? 0 : t > last ? nstate - 1 : (size_t)path[t];
        low[t] = p > halfwidth ? p - halfwidth : 0;
        high[t] = (halfwidth >= nstate || p + halfwidth + 1 > nstate) ? nstate : p + halfwidth + 1;
    }
    low[0] = 0;
    high[nblock - 1] = nstate;
    return 0;
}

/* the library defines it (scrappie_hip.hip); weak, so that this file also links into the host-only builds of the tests */
void sh_set_error(const char *fmt, ...) __attribute__((weak, format(printf, 1, 2)));
#define SH_ERR(...) do { if (sh_set_error) sh_set_error(__VA_ARGS__); } while (0)

static int base_code(char b) {
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return -1;
    }
}

/* the state code of every window of state_len bases (oldest base most significant), n - state_len + 1 of them, calloc'd.
 * One pass: a window's code is the previous one without its oldest base, times four, plus the new base -- in unsigned
 * arithmetic, which wraps exactly as the reference's int products do for long windows.  NULL (and the reason in
 * scrappie_hip_last_error) on a base outside ACGT / acgt, or when there is no whole window. */
int *encode_bases_to_integers(char const *seq, size_t n, size_t state_len) {
    if (!seq || state_len == 0) { SH_ERR("encode_bases_to_integers: no sequence or a zero state length"); return NULL; }
    if (n < state_len) { SH_ERR("encode_bases_to_integers: %zu bases hold no window of %zu", n, state_len); return NULL; }
    for (size_t i = 0; i < n; i++)
        if (base_code(seq[i]) < 0) {
            warnx("Unrecognised base %d in read", seq[i]);
            SH_ERR("encode_bases_to_integers: unrecognised base %d at %zu", seq[i], i);
            return NULL;
        }
    const size_t nstate = n - state_len + 1;
    int *codes = calloc(nstate, sizeof(int));
    if (!codes) { SH_ERR("encode_bases_to_integers: out of memory"); return NULL; }
    unsigned top = 1;                        /* weight of the oldest base: 4^(state_len - 1), mod 2^32 */
    for (size_t j = 1; j < state_len; j++) top *= 4u;
    unsigned code = 0;
    for (size_t j = 0; j < state_len; j++) code = code * 4u + (unsigned)base_code(seq[j]);
    codes[0] = (int)code;
    for (size_t i = 1; i < nstate; i++) {
        code = (code - (unsigned)base_code(seq[i - 1]) * top) * 4u + (unsigned)base_code(seq[i + state_len - 1]);
        codes[i] = (int)code;
    }
    return codes;
}

/* ------------------------------------------------------------------ */
/* squiggle matching: the per-position tables (decode.c:1055-1099)      */
/* ------------------------------------------------------------------ */
/* What squiggle_match_viterbi / _forward compute before their sample loop, with the reference's expressions and its
 * summation order, from the same libm: tab = loc[npos] | scale[npos] | logsc[npos] | move_pen[npos + 2] | stay_pen[npos + 2]
 * (the means in the START and END slots); pens = { logf(prob_back), logf(0.5f) }.  params: npos columns of ldp floats
 * (mean, log sd, dwell logit). */
void sh_squiggle_tables(const float *params, size_t npos, size_t ldp, float rate, float prob_back, float *tab, float pens[2]) {
    float *loc = tab, *scale = tab + npos, *logsc = tab + 2 * npos, *move_pen = tab + 3 * npos, *stay_pen = tab + 4 * npos + 2;
    const size_t nfstate = npos + 2;
    pens[0] = logf(prob_back);
    pens[1] = logf(0.5f);
    for (size_t pos = 0; pos < npos; pos++) {
        loc[pos] = params[pos * ldp + 0];
        logsc[pos] = params[pos * ldp + 1];
        scale[pos] = expf(params[pos * ldp + 1]);
    }
    const float lograte = logf(rate);
    float mean_move_pen = 0.0f;
    float mean_stay_pen = 0.0f;
    for (size_t pos = 0; pos < npos; pos++) {
        const float x = params[pos * ldp + 2] + lograte;
        const float mp = (1.0f - prob_back) * (0.5f * (1.0f + tanhf(x / 2.0f)));      /* plogisticf, util.h:110-112 */
        move_pen[pos + 1] = logf(mp);
        stay_pen[pos + 1] = log1pf(-mp - prob_back);
        mean_move_pen += move_pen[pos + 1];
        mean_stay_pen += stay_pen[pos + 1];
    }
    mean_move_pen /= npos;
    mean_stay_pen /= npos;
    move_pen[0] = mean_move_pen;
    move_pen[nfstate - 1] = mean_move_pen;
    stay_pen[0] = mean_stay_pen;
    stay_pen[nfstate - 1] = mean_stay_pen;
}

/* ------------------------------------------------------------------ */
/* event detection (event_detection.c)                                  */
/* ------------------------------------------------------------------ */
/* The host statement of detect_events: what the kernels of sh_events.h are held against bit for bit, and the reference's
 * arithmetic with its types and its order of operations kept (no contraction: -ffp-contract=off).
 *   running sums: sequential double additions of (double)x and (double)(x * x), the product rounded to float first;
 *   t-statistic: window sums as double differences, the first window's mean and mean square divided in double and narrowed, the
 *     second window's in float; the pooled variance summed left to right in double, narrowed, clamped at FLT_MIN, divided by w in
 *     float; the statistic a double division by a double square root, narrowed;
 *   peaks: the short and the long detector walk the two statistics together, the short one masking the long one; peaks are kept
 *     in the order they are emitted;
 *   events: cut at the peaks from the running sums; the length of an event is (float) of an unsigned 64-bit difference, which
 *     wraps for a pair of peaks out of order, as the reference's size_t arithmetic does. */
#include <float.h>

const detector_param event_detection_defaults = {3, 6, 1.4f, 9.0f, 0.2f};

void sh_event_sums(const float *x, size_t n, double *sum, double *sumsq) {
    sum[0] = 0.0; sumsq[0] = 0.0;
    for (size_t i = 0; i < n; i++) {
        const float sq = x[i] * x[i];
        sum[i + 1] = sum[i] + (double)x[i];
        sumsq[i + 1] = sumsq[i] + (double)sq;
    }
}

void sh_event_tstat(const double *sum, const double *sumsq, size_t n, size_t w, float *t) {
    for (size_t i = 0; i < n; i++) t[i] = 0.0f;
    if (n < 2 * w || w < 2) return;
    const float wf = (float)w;
    for (size_t i = w; i <= n - w; i++) {
        double sum1 = sum[i], sumsq1 = sumsq[i];
        if (i > w) { sum1 -= sum[i - w]; sumsq1 -= sumsq[i - w]; }
        const float sum2 = (float)(sum[i + w] - sum[i]);
        const float sumsq2 = (float)(sumsq[i + w] - sumsq[i]);
        const float mean1 = (float)(sum1 / (double)wf);
        const float mean2 = sum2 / wf;
        const float m1sq = mean1 * mean1, m2sq = mean2 * mean2, msq2 = sumsq2 / wf;
        double cv = sumsq1 / (double)wf - (double)m1sq;
        cv = cv + (double)msq2;
        cv = cv - (double)m2sq;
        const float var = fmaxf((float)cv, FLT_MIN);
        const float dm = mean2 - mean1;
        const float vw = var / wf;
        t[i] = (float)(fabs((double)dm) / sqrt((double)vw));
    }
}

typedef struct { uint64_t masked_to; int64_t peak_pos; float peak_value, threshold; uint64_t window; int valid; } sh_detector;

/* peaks[] takes at most n positions; returns their number */
size_t sh_event_peaks(const float *t1, const float *t2, size_t n, const detector_param *p, uint32_t *peaks) {
    sh_detector d[2] = {{0, -1, FLT_MAX, p->threshold1, p->window_length1, 0}, {0, -1, FLT_MAX, p->threshold2, p->window_length2, 0}};
    const float *sig[2] = {t1, t2};
    const float height = p->peak_height;
    size_t np = 0;
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 2; k++) {
            sh_detector *q = &d[k];
            if (q->masked_to >= i) continue;
            const float v = sig[k][i];
            if (q->peak_pos < 0) {
                if (v < q->peak_value) q->peak_value = v;                       /* a deeper minimum */
                else if (v - q->peak_value > height) { q->peak_value = v; q->peak_pos = (int64_t)i; }
            } else {
                if (v > q->peak_value) { q->peak_value = v; q->peak_pos = (int64_t)i; }
                if (k == 0 && q->peak_value > q->threshold) {                   /* the short detector will fire: the long one starts over behind it */
                    d[1].masked_to = (uint64_t)q->peak_pos + q->window;
                    d[1].peak_pos = -1; d[1].peak_value = FLT_MAX; d[1].valid = 0;
                }
                if (q->peak_value - v > height && q->peak_value > q->threshold) q->valid = 1;
                if (q->valid && (uint64_t)((int64_t)i - q->peak_pos) > q->window / 2) {
                    if (np < n) peaks[np++] = (uint32_t)q->peak_pos;      /* (a detector fires at most every other sample: np <= n; the test keeps absurd parameters inside the list too) */
                    q->peak_pos = -1; q->peak_value = v; q->valid = 0;
                }
            }
        }
    return np;
}

event_t sh_event_make(uint64_t start, uint64_t end, const double *sum, const double *sumsq) {
    event_t ev;
    memset(&ev, 0, sizeof ev);            /* (the struct's tail padding too: tables are compared as bytes) */
    ev.pos = -1; ev.state = -1;
    ev.start = start;
    ev.length = (float)(end - start);
    ev.mean = (float)(sum[end] - sum[start]) / ev.length;
    const float dsq = (float)(sumsq[end] - sumsq[start]);
    const float msq = ev.mean * ev.mean;
    const float var = dsq / ev.length - msq;
    ev.stdv = sqrtf(fmaxf(var, 0.0f));
    return ev;
}

/* detect_events on x[0 .. n): .event == NULL where no event table exists (no peak: the reference reads peaks[-1] there; no samples; out of
 * memory).  tstat1 / tstat2 (may be NULL): n floats each, the two statistics. */
event_table scrappie_hip_detect_events_host(const float *x, size_t n, const detector_param *param, float *tstat1, float *tstat2) {
    event_table et = {0, 0, 0, NULL};
    const detector_param p = param ? *param : event_detection_defaults;
    if (!x || n == 0 || n > (size_t)UINT32_MAX - 1) return et;
    double *sum = malloc((n + 1) * sizeof(double)), *sumsq = malloc((n + 1) * sizeof(double));
    float *t1 = malloc(n * sizeof(float)), *t2 = malloc(n * sizeof(float));
    uint32_t *peaks = malloc(n * sizeof(uint32_t));
    if (sum && sumsq && t1 && t2 && peaks) {
        sh_event_sums(x, n, sum, sumsq);
        sh_event_tstat(sum, sumsq, n, p.window_length1, t1);
        sh_event_tstat(sum, sumsq, n, p.window_length2, t2);
        if (tstat1) memcpy(tstat1, t1, n * sizeof(float));
        if (tstat2) memcpy(tstat2, t2, n * sizeof(float));
        const size_t np = sh_event_peaks(t1, t2, n, &p, peaks);
        if (np > 0 && (et.event = malloc((np + 1) * sizeof(event_t))) != NULL) {
            for (size_t k = 0; k <= np; k++)
                et.event[k] = sh_event_make(k ? peaks[k - 1] : 0, k < np ? peaks[k] : n, sum, sumsq);
            et.n = np + 1; et.start = 0; et.end = np + 1;
        }
    }
    free(peaks); free(t2); free(t1); free(sumsq); free(sum);
    return et;
}
