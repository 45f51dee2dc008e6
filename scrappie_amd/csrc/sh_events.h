/* sh_events.h -- event detection on the device: detect_events of event_detection.c for a batch of reads, bit-identical to the host
 * statement in sh_host.c (scrappie_hip_detect_events_host) and so to the reference.  Four kernels, split by what is serial:
 *
 *   k_ev_sums    running sums of x and of float(x * x) in double.  Double addition is not associative and the reference adds in sample
 *                order, so a read is ONE serial chain: one lane per read, 64 reads per wave.  The samples reach the lanes through LDS:
 *                the wave loads SH_EV_TILE consecutive samples of each of its reads with coalesced loads (a row of 128 bytes per read),
 *                every lane then walks its own row, and the sums leave the same way.  No lane ever touches a cache line of its own.
 *   k_ev_tstat   the two Welch statistics, one thread per sample of every read: all the expensive arithmetic (three double divisions,
 *                three float divisions and a double square root per sample and window) is here, and it is parallel.
 *   k_ev_peaks   the short / long peak detector.  The two detectors mask each other and carry their state from sample to sample, so
 *                this is serial per read again: one lane per read, the two statistics staged through LDS like the samples, the
 *                detectors' state in registers, peaks appended to the read's own list in the order they are emitted.
 *   k_ev_events  one thread per event: the sums gathered at the two peaks that bound it, event_t written.
 *
 * Scratch per sample slot: two doubles (sums), two floats (statistics), one uint32 (peak) = 28 bytes; read i owns n_i + 1 slots from
 * ShEvRead::slot in each array (the sums have n + 1 entries; the other arrays leave their last slot unused).
 *
 * Arithmetic.  Every operation is the reference's, in its type and order; the translation unit is compiled with -ffp-contract=off, so
 * nothing is fused.  `/` and sqrt on double, and `/` and sqrtf on float, are what the compiler makes of them for gfx950: the division
 * expansions (v_div_scale / v_div_fmas / v_div_fixup) and the f64 square root (v_rsq_f64 refined with fma residual steps) are correctly
 * rounded, float denormals are kept (FLT_MIN / w is one), and the fixtures of tests/golden/events/ref_event_detect.npz hold all of them to the
 * reference's x86 results bit for bit.
 *
 * LDS layout (cdna_hip_programming.md section 2): a tile is [64 reads][SH_EV_TILE + 1] -- rows padded by one access width, so that the
 * 64 lanes of the walk (lane = read, all at the same column) fall on distinct banks for floats (stride 33 dwords), and on the inherent
 * two passes for doubles (64 lanes x 8 bytes through 32 banks of ds_write_b64).  Filling and draining a tile go along the rows. */
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include "scrappie_hip.h"

#define SH_EV_TILE 32          /* samples per read of one staged tile */
#define SH_EV_READS 64         /* reads per workgroup of the serial kernels: one wave, one lane per read */
#define SH_EV_MAX_WINDOW 4096  /* window lengths the batch accepts (the reference's defaults: 3 and 6) */

struct ShEvRead {
    long long sig;      /* first sample of the read in the launch's signal buffer */
    long long slot;     /* first slot of the read in the scratch arrays */
    int n;              /* samples */
    int pad_;
};

struct ShEvParams { int w1, w2; float threshold1, threshold2, peak_height; };

/* the records of a workgroup's 64 reads, in LDS for the fill / drain loops */
struct ShEvWave { long long sig[SH_EV_READS], slot[SH_EV_READS]; int n[SH_EV_READS]; };

static __device__ __forceinline__ int ev_wave_setup(const ShEvRead *rd, int nread, ShEvWave &w) {
    const int lane = (int)threadIdx.x, me = (int)blockIdx.x * SH_EV_READS + lane;
    const bool live = me < nread;
    w.sig[lane] = live ? rd[me].sig : 0;
    w.slot[lane] = live ? rd[me].slot : 0;
    const int n = live ? rd[me].n : 0;
    w.n[lane] = n;
    int nmax = n;
    for (int d = 32; d; d >>= 1) nmax = max(nmax, __shfl_xor(nmax, d));
    __syncthreads();
    return nmax;
}

/* SH_EV_TILE samples from t0 on of each of the workgroup's reads, from NS arrays at once: src[k][first[r] + t0 + j] -> tile[k][r][j].  Rows of
 * reads that have ended (and of lanes past the launch: n = 0) get zeros, which nobody reads.  All the loads of a tile are issued
 * before the first of them is waited for (the loops are unrolled: SH_EV_READS / 2 loads per lane and array in flight); written as one loop
 * with the store behind its load, a tile costs that many memory latencies one after the other. */
template <int NS, class T>
static __device__ __forceinline__ void ev_fill(const T *const (&src)[NS], const long long *first, const int *n, int t0, T (*const (&tile)[NS])[SH_EV_TILE + 1]) {
    constexpr int STEP = SH_EV_READS / SH_EV_TILE, NIT = SH_EV_READS / STEP;
    const int lane = (int)threadIdx.x, j = lane % SH_EV_TILE, r0 = lane / SH_EV_TILE;
    T v[NS][NIT];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int r = r0 + it * STEP;
        const bool live = t0 + j < n[r];
        const long long at = first[r] + t0 + j;
#pragma unroll
        for (int k = 0; k < NS; k++) v[k][it] = live ? src[k][at] : T(0);
    }
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int r = r0 + it * STEP;
#pragma unroll
        for (int k = 0; k < NS; k++) tile[k][r][j] = v[k][it];
    }
}
/* ... and back: tile[r][j] -> dst[first[r] + shift + t0 + j] */
template <class T>
static __device__ __forceinline__ void ev_drain(T *dst, const long long *first, const int *n, int t0, int shift, const T (*tile)[SH_EV_TILE + 1]) {
    constexpr int STEP = SH_EV_READS / SH_EV_TILE;
    const int lane = (int)threadIdx.x, j = lane % SH_EV_TILE, r0 = lane / SH_EV_TILE;
#pragma unroll
    for (int it = 0; it < SH_EV_READS / STEP; it++) {
        const int r = r0 + it * STEP;
        if (t0 + j < n[r]) dst[first[r] + shift + t0 + j] = tile[r][j];
    }
}

__global__ void __launch_bounds__(SH_EV_READS) k_ev_sums(const ShEvRead *rd, int nread, const float *sig, double *sum, double *sumsq) {
    __shared__ ShEvWave w;
    __shared__ float xs[SH_EV_READS][SH_EV_TILE + 1];
    __shared__ double ss[SH_EV_READS][SH_EV_TILE + 1], qs[SH_EV_READS][SH_EV_TILE + 1];
    const int lane = (int)threadIdx.x;
    const int nmax = ev_wave_setup(rd, nread, w);
    const int n = w.n[lane];
    double s = 0.0, q = 0.0;
    if (n > 0) { sum[w.slot[lane]] = 0.0; sumsq[w.slot[lane]] = 0.0; }
    for (int t0 = 0; t0 < nmax; t0 += SH_EV_TILE) {
        ev_fill<1, float>({sig}, w.sig, w.n, t0, {xs});
        __syncthreads();
        const int m = min(SH_EV_TILE, n - t0);      /* (<= 0 for a read that has ended) */
        const auto step = [&](int j) {
            const float x = xs[lane][j];
            const float sq = x * x;                 /* rounded to float before it is widened, as the reference's data[i] * data[i] */
            s = s + (double)x;
            q = q + (double)sq;
            ss[lane][j] = s; qs[lane][j] = q;
        };
        if (m == SH_EV_TILE) {                      /* a whole tile: unrolled, the row's LDS reads ahead of the chain of additions */
#pragma unroll
            for (int j = 0; j < SH_EV_TILE; j++) step(j);
        } else
            for (int j = 0; j < m; j++) step(j);
        __syncthreads();
        ev_drain(sum, w.slot, w.n, t0, 1, ss);
        ev_drain(sumsq, w.slot, w.n, t0, 1, qs);
        __syncthreads();
    }
}

/* compute_tstat at sample i of a read of n samples; sum / sumsq: the read's n + 1 running sums */
static __device__ __forceinline__ float ev_tstat(const double *sum, const double *sumsq, int n, int w, int i) {
    if (w < 2 || n < 2 * w || i < w || i > n - w) return 0.0f;
    const float wf = (float)w;
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
    return (float)(fabs((double)dm) / sqrt((double)vw));
}

/* the read that owns slot g: the last record whose first slot is <= g (the records' slots ascend) */
static __device__ __forceinline__ int ev_find_read(const ShEvRead *rd, int nread, long long g) {
    int lo = 0, hi = nread - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rd[mid].slot <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_ev_tstat(const ShEvRead *rd, int nread, long long nslot, const double *sum, const double *sumsq,
                                                  float *t1, float *t2, ShEvParams p) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= nslot) return;
    const int r = ev_find_read(rd, nread, g);
    const long long first = rd[r].slot;
    const int n = rd[r].n, i = (int)(g - first);
    if (i >= n) return;                            /* the sums' last slot */
    t1[g] = ev_tstat(sum + first, sumsq + first, n, p.w1, i);
    t2[g] = ev_tstat(sum + first, sumsq + first, n, p.w2, i);
}

/* one detector of short_long_peak_detector */
struct ShEvDetector { long long masked_to, peak_pos; float peak_value; bool valid; };

__global__ void __launch_bounds__(SH_EV_READS) k_ev_peaks(const ShEvRead *rd, int nread, const float *t1, const float *t2, unsigned *peaks,
                                                         int *npeak, ShEvParams p) {
    __shared__ ShEvWave w;
    __shared__ float a1[SH_EV_READS][SH_EV_TILE + 1], a2[SH_EV_READS][SH_EV_TILE + 1];
    const int lane = (int)threadIdx.x, me = (int)blockIdx.x * SH_EV_READS + lane;
    const int nmax = ev_wave_setup(rd, nread, w);
    const int n = w.n[lane];
    unsigned *mine = peaks + w.slot[lane];
    ShEvDetector d[2] = {{0, -1, FLT_MAX, false}, {0, -1, FLT_MAX, false}};
    const float thr[2] = {p.threshold1, p.threshold2};
    const long long win[2] = {p.w1, p.w2};
    int np = 0;
    for (int t0 = 0; t0 < nmax; t0 += SH_EV_TILE) {
        ev_fill<2, float>({t1, t2}, w.slot, w.n, t0, {a1, a2});
        __syncthreads();
        const int m = min(SH_EV_TILE, n - t0);
        for (int j = 0; j < m; j++) {
            const long long i = t0 + j;
            const float cur[2] = {a1[lane][j], a2[lane][j]};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                ShEvDetector &q = d[k];
                if (q.masked_to >= i) continue;
                const float v = cur[k];
                if (q.peak_pos < 0) {
                    if (v < q.peak_value) q.peak_value = v;
                    else if (v - q.peak_value > p.peak_height) { q.peak_value = v; q.peak_pos = i; }
                } else {
                    if (v > q.peak_value) { q.peak_value = v; q.peak_pos = i; }
                    if (k == 0 && q.peak_value > thr[0]) {
                        d[1].masked_to = q.peak_pos + win[0];
                        d[1].peak_pos = -1; d[1].peak_value = FLT_MAX; d[1].valid = false;
                    }
                    if (q.peak_value - v > p.peak_height && q.peak_value > thr[k]) q.valid = true;
                    if (q.valid && i - q.peak_pos > win[k] / 2) {
                        if (np < n) mine[np++] = (unsigned)q.peak_pos;        /* a detector fires at most every other sample, so np <= n: inside the read's slots */
                        q.peak_pos = -1; q.peak_value = v; q.valid = false;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (me < nread) npeak[me] = np;
}

/* Event e of the launch: read r = the one whose [ev_off[r], ev_off[r + 1]) holds e, event k = e - ev_off[r] of its npeak + 1: bounded by
 * peaks k - 1 and k (0 and n at the ends).  The length is (float) of an unsigned 64-bit difference: it wraps for peaks out of order, as the
 * reference's size_t arithmetic does. */
__global__ void __launch_bounds__(256) k_ev_events(const ShEvRead *rd, int nread, const long long *ev_off, const double *sum, const double *sumsq,
                                                   const unsigned *peaks, uint4 *out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= ev_off[nread]) return;
    int lo = 0, hi = nread - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ev_off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    /* (reads without events have ev_off[r] == ev_off[r + 1]: the search lands on the last record that starts at or before e, which has events) */
    const int r = lo;
    const long long first = rd[r].slot;
    const int k = (int)(e - ev_off[r]), nev = (int)(ev_off[r + 1] - ev_off[r]);
    const uint64_t start = k ? peaks[first + k - 1] : 0, end = k < nev - 1 ? peaks[first + k] : (uint64_t)rd[r].n;
    const float length = (float)(end - start);
    const float mean = (float)(sum[first + end] - sum[first + start]) / length;
    const float dsq = (float)(sumsq[first + end] - sumsq[first + start]);
    const float msq = mean * mean;
    const float var = dsq / length - msq;
    const float stdv = sqrtf(fmaxf(var, 0.0f));
    static_assert(sizeof(event_t) == 32, "event_t layout");
    out[2 * e] = make_uint4((unsigned)start, (unsigned)(start >> 32), __float_as_uint(length), __float_as_uint(mean));
    out[2 * e + 1] = make_uint4(__float_as_uint(stdv), 0xffffffffu, 0xffffffffu, 0u);      /* stdv, pos = -1, state = -1, padding */
}
