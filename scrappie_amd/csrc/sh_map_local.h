/* sh_map_local.h -- part of sh_kernels.h (included from there, behind sh_map_crf_local.h): a read of a transducer model mapped INTO a
 * longer sequence of k-mer states: where in the sequence the read lies, with what score and along what path.  The reference has
 * no such function; the definition is map_to_sequence_viterbi / _forward (decode.c:1420-1640, unbanded; k_map, sh_map.h) with the
 * sequence side made local.
 *
 * States: the positions 0 .. L - 1, START, and one END accumulator E[pos] per position.  Before block 0 START = 0 and everything
 * else -SH_MAP_BIG.  Block t, previous row p to c, lps the block's stay entry, le(pos) the entry of state seq[pos],
 * ls = fmaxf(-local_pen, lps):
 *   c[START] = p[START] + ls
 *   c[pos]   = (p[pos] - stay_pen) + lps, then on strict > in this order: step p[pos - 1] + le (pos >= 1), skip
 *              (p[pos - 2] - skip_pen) + le (pos >= 2), from START p[START] + le -- for EVERY pos (the reference: pos 0 only)
 *   E'[pos]  = E[pos] + ls, then p[pos] - local_pen on strict >: any position may leave for END (the reference: L - 1 only)
 * End: x the first maximum of c[pos], y the first maximum of E[pos], pos ascending; the score fmaxf(x, y); the path ends in a
 * sequence cell iff x > y (decode.c:1512-1514).  START is no end state.  Forward: sh_lse in place of every max and strict >.
 * path[blk] (nblock entries): the position in seq, -1 in START / END; first the lowest position visited, last the highest + 1.
 * At pos 0 the cell is the reference's operation for operation, and every global path is a local one: the score is never below
 * map_to_sequence_viterbi's.
 *
 * Windows.  A path enters the sequence from START exactly once and advances at most 2 positions per block.  Window w of stride s
 * OWNS the paths whose entry position lies in [w s, min((w + 1) s, L)): only those cells take the START move.  Its cells are
 * [w s, min(w s + s - 1 + 2 (nblock - 1), L - 1)]; a cell left of the window reads as -SH_MAP_BIG.  Every path is owned by exactly
 * one window and lies inside it, and its score is the same chain of float additions wherever it is computed: the Viterbi score is
 * bit-identical for every stride, one window included.  The host takes the highest window (the lowest on a tie), or sh_lse over
 * the windows in their order.  The cut is host arithmetic: scrappie_hip_map_local_plan (sh_host.c).
 *
 * Work split: one workgroup of SH_MAP_NTH threads per (read, window), cell j of the window on thread j % SH_MAP_NTH, two
 * ping-pong score rows and one barrier per block as k_map; E is a third row that only a cell's own thread touches; START is
 * the same chain of additions in every thread's register.
 *
 * The posterior column in LDS.  k_map gathers one posterior entry per cell from HBM and finalises it there; a window of a long
 * sequence touches every state many times.  Here the workgroup loads the read's whole column of a block -- ceil(nr / 4) pieces of
 * 16 bytes, piece q on thread q % SH_MAP_NTH; tiled: from E + sums through ShMapPost<true>'s address arithmetic, dense: the row of
 * the uploaded matrix --, finalises every entry once with the fin_post(v, d_rcp(sum), min_prob, 1 - min_prob, 1) call k_map makes
 * (so the DP sees the bits scrappie_hip_posterior returns) and writes it to a double-buffered LDS column; the cells read
 * col[seq[pos]] from LDS.  The loads of block t + 1 are issued before the cells of block t and written behind them, before block
 * t's barrier; they are unconditional (clamped block and piece index, no lane condition).  SH_MAPL_PIECES pieces per thread:
 * at most 4 * SH_MAP_NTH * SH_MAPL_PIECES states.
 *
 * Homes: rows, E, codes, two columns and the head fit SH_MAP_LDS -- (SH_MAPL_HEAD + 2 nrp + 4 RW) words, nrp = 4 ceil(nr / 4),
 * RW = 4 ceil(ncell / 4) -- or the three rows live in device scratch (3 RW floats; the codes are then read from the sequence):
 * two instantiations, two launches, never a pointer that chooses at run time.
 *
 * Traceback (the second pass, on a read's best window alone): k_map's 2-bit move codes in its ballot layout, indexed by the cell
 * IN the window, W = 4 ceil(ncell / 64) words per block; behind all of them one more ballot plane, "E took the fresh value this
 * block", W / 2 words per block.  Per wave whole words, plain vector stores.  k_map_local_walk, one thread per read: path, first,
 * last.
 *
 * End of a window: every thread scans its cells in order, then six __shfl_xor steps inside the wave, then the four waves through
 * LDS, thread 0 last; once for the c row and once for E.  Viterbi carries (score, j): the higher score, on equal scores the lower
 * j -- the first maximum whatever the order.  Forward: acc = -SH_MAP_BIG, sh_lse(acc, v) per cell, sh_lse(acc, __shfl_xor(acc, d))
 * for d = 1 .. 32, then waves 0 .. 3 in order; the score sh_lse(x, y). */
#ifndef SH_MAP_LOCAL_H
#define SH_MAP_LOCAL_H

#include "sh_map.h"

#define SH_MAPL_HEAD 32         /* words in front of the columns: the waves' results of the end reduction */
#define SH_MAPL_PIECES 2        /* 16-byte pieces of a column per thread: 2048 states at most */

struct ShMapLocalWin {
    long long post;     /* dense: float offset of the read's row 0; tiled: the read's first column block */
    long long tb;       /* first traceback word (multiple of 4); -1: no traceback */
    long long scr;      /* float offset of the three rows in device scratch; -1: in LDS */
    long long seq;      /* offset of the sequence's code 0 */
    int nblock, seqlen;
    int lane;           /* tiled: the read's lane in its tile (0..15) */
    int first;          /* the window's first cell (a position in the sequence) */
    int ncell;          /* its cells: first .. first + ncell - 1 < seqlen */
    int own;            /* the entry positions it owns: first .. first + own - 1 */
    int ok;             /* 0: nothing to do */
    int pad_;
};

struct ShMapLocalArgs {
    const ShMapLocalWin *rd;
    const float *post;          /* dense posterior */
    const float *E, *sums;      /* tiled posterior */
    long long pstride;          /* dense: floats per row (a multiple of 4, at least 4 ceil(nr / 4)) */
    int nr;                     /* states, stay included */
    int nchunk;                 /* tiled: chunks of 16 states per column block */
    float min_prob;             /* tiled: fin_post's floor */
    float stay_pen, skip_pen, local_pen;
    const int *seq;
    unsigned *tb;
    float *scr;
    float *score;               /* [window] */
    int2 *final_state;          /* [window] Viterbi: (the end position, 1: the path ends in its E, 0: in the cell) */
};

__device__ __forceinline__ int sh_map_local_words(int ncell) { return 4 * ((ncell + 63) / 64); }

/* the 16-byte pieces of a read's column of one block, and what finalises them */
template <bool TILED> struct ShMapLocalCol;
template <> struct ShMapLocalCol<false> {
    const float *base; long long pstride;
    __device__ __forceinline__ ShMapLocalCol(const ShMapLocalArgs &a, const ShMapLocalWin &r) : base(a.post + r.post), pstride(a.pstride) {}
    __device__ __forceinline__ float4 piece(int blk, int q) const { return *(const float4 *)(base + (long long)blk * pstride + 4 * q); }
    __device__ __forceinline__ float scale(int) const { return 0.0f; }
    __device__ __forceinline__ float4 fin(float4 v, float) const { return v; }
};
template <> struct ShMapLocalCol<true> {
    const float *base, *sums; long long cstride; float mp, mpm1;
    __device__ __forceinline__ ShMapLocalCol(const ShMapLocalArgs &a, const ShMapLocalWin &r)
        : base(a.E + r.post * a.nchunk * 256 + r.lane * 4), sums(a.sums + r.post * 16 + r.lane), cstride((long long)a.nchunk * 256), mp(a.min_prob),
          mpm1(1.0f - a.min_prob) {}
    /* states 4 q .. 4 q + 3: ShMapPost<true>'s (s >> 4) * 256 + ((s >> 2) & 3) * 64 + (s & 3) */
    __device__ __forceinline__ float4 piece(int blk, int q) const { return *(const float4 *)(base + blk * cstride + (q >> 2) * 256 + (q & 3) * 64); }
    __device__ __forceinline__ float scale(int blk) const { return sums[(long long)blk * 16]; }
    __device__ __forceinline__ float4 fin(float4 v, float sum) const {
        const float rcp = d_rcp(sum);
        return make_float4(fin_post(v.x, rcp, mp, mpm1, 1), fin_post(v.y, rcp, mp, mpm1, 1), fin_post(v.z, rcp, mp, mpm1, 1), fin_post(v.w, rcp, mp, mpm1, 1));
    }
};

/* One sequence cell: k_map's (sh_map_cell) with the START move for every owned cell and neighbours given by value -- p0, p1, p2
 * the previous row at the cell, one and two to its left (-SH_MAP_BIG left of the window), ps START.  The reference's expressions
 * in its order -- stay, step, skip, START -- with strict > (code: the move taken) or sh_lse. */
template <bool VIT>
__device__ __forceinline__ float sh_map_local_cell(float p0, float p1, float p2, float ps, int pos, bool mine, float le, float lps, float stay_pen,
                                                   float skip_pen, int &code) {
    float v = (p0 - stay_pen) + lps;
    if (VIT) {
        int c = 0;
        if (pos >= 1) { const float st = p1 + le; if (st > v) { v = st; c = 1; } }
        if (pos >= 2) { const float sk = (p2 - skip_pen) + le; if (sk > v) { v = sk; c = 2; } }
        if (mine) { const float fs = ps + le; if (fs > v) { v = fs; c = 3; } }
        code = c;
    } else {
        if (pos >= 1) v = sh_lse(v, p1 + le);
        if (pos >= 2) v = sh_lse(v, (p2 - skip_pen) + le);
        if (mine) v = sh_lse(v, ps + le);
    }
    return v;
}

/* first maximum (VIT: score and key, the lower key on equal scores) or sh_lse of acc over the workgroup; res: 8 words of LDS; every
 * thread returns with thread 0 holding the result */
template <bool VIT>
__device__ __forceinline__ void sh_map_local_reduce(float &acc, int &key, float *res, int tid) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float ov = __shfl_xor(acc, d);
        if (VIT) {
            const int ok = __shfl_xor(key, d);
            if (ov > acc || (ov == acc && ok < key)) { acc = ov; key = ok; }
        } else {
            acc = sh_lse(acc, ov);
        }
    }
    const int wv = tid >> 6;
    if ((tid & 63) == 0) { res[wv] = acc; ((int *)res)[4 + wv] = key; }
    __syncthreads();
    if (tid == 0) {
        acc = res[0]; key = ((const int *)res)[4];
        for (int w = 1; w < SH_MAP_NTH / 64; w++) {
            const float ov = res[w];
            const int ok = ((const int *)res)[4 + w];
            if (VIT) { if (ov > acc || (ov == acc && ok < key)) { acc = ov; key = ok; } }
            else acc = sh_lse(acc, ov);
        }
    }
}

template <bool VIT, bool TILED, bool LDS>
__global__ __launch_bounds__(SH_MAP_NTH) void k_map_local(ShMapLocalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_mapl_lds2[];
    const ShMapLocalWin r = a.rd[blockIdx.x];
    if (!r.ok) return;
    const int tid = threadIdx.x, NB = r.nblock, NC = r.ncell, c0 = r.first, RW = (NC + 3) & ~3;
    const int NP = (a.nr + 3) >> 2, NRP = NP * 4, STAY = a.nr - 1;
    const float stay_pen = a.stay_pen, skip_pen = a.skip_pen, local_pen = a.local_pen;
    float *const res = sh_mapl_lds2;                          /* [SH_MAPL_HEAD] */
    float *const col0 = sh_mapl_lds2 + SH_MAPL_HEAD;          /* [2][NRP] */
    float *const buf0 = LDS ? col0 + 2 * NRP : a.scr + r.scr;
    float *const buf1 = buf0 + RW;
    float *const erow = buf1 + RW;
    int *const lds_seq = (int *)(col0 + 2 * NRP + 3 * RW);
    const int *const gseq = a.seq + r.seq + c0;
    if (LDS)
        for (int j = tid; j < NC; j += SH_MAP_NTH) lds_seq[j] = gseq[j];
    for (int j = tid; j < NC; j += SH_MAP_NTH) { buf0[j] = -SH_MAP_BIG; erow[j] = -SH_MAP_BIG; }
    const ShMapLocalCol<TILED> cl(a, r);
    /* piece q[k] of this thread: tid + k * SH_MAP_NTH, clamped to the column's last */
    int pq[SH_MAPL_PIECES];
    float4 q[SH_MAPL_PIECES];
#pragma unroll
    for (int k = 0; k < SH_MAPL_PIECES; k++) pq[k] = min(tid + k * SH_MAP_NTH, NP - 1);
    {
        const float sum = cl.scale(0);
#pragma unroll
        for (int k = 0; k < SH_MAPL_PIECES; k++) {
            const float4 f = cl.fin(cl.piece(0, pq[k]), sum);
            if (tid + k * SH_MAP_NTH < NP) *(float4 *)(col0 + 4 * pq[k]) = f;
        }
    }
    const bool want_tb = VIT && r.tb >= 0;
    const int W = sh_map_local_words(NC);
    unsigned *const tbw = want_tb ? a.tb + r.tb : nullptr;
    unsigned *const tbe = want_tb ? tbw + (long long)NB * W : nullptr;
    const int wv = tid >> 6;
    const int nch = (NC + SH_MAP_NTH - 1) / SH_MAP_NTH;
    float start = 0.0f;                                      /* START before block t: the same in every thread */
    __syncthreads();
    for (int t = 0; t < NB; t++) {
        const float *const p = (t & 1) ? buf1 : buf0;
        float *const c = (t & 1) ? buf0 : buf1;
        const float *const col = col0 + (t & 1) * NRP;
        const int tn = min(t + 1, NB - 1);                   /* block t + 1's column: issued now, written behind the cells */
        const float sumn = cl.scale(tn);
#pragma unroll
        for (int k = 0; k < SH_MAPL_PIECES; k++) q[k] = cl.piece(tn, pq[k]);
        const float lps = col[STAY];
        const float ls = VIT ? fmaxf(-local_pen, lps) : sh_lse(-local_pen, lps);
        for (int ch = 0; ch < nch; ch++) {
            const int j = ch * SH_MAP_NTH + tid, pos = c0 + j;
            const bool valid = j < NC;
            const int j0 = min(j, NC - 1), j1 = max(j0 - 1, 0), j2 = max(j0 - 2, 0);
            const int s = LDS ? lds_seq[j0] : gseq[j0];
            const float le = col[s];
            const float p0 = p[j0], l1 = p[j1], l2 = p[j2];
            const float p1 = j >= 1 ? l1 : -SH_MAP_BIG, p2 = j >= 2 ? l2 : -SH_MAP_BIG;      /* left of the window: no owned path */
            int code = 0;
            const float v = sh_map_local_cell<VIT>(p0, p1, p2, start, pos, j < r.own, le, lps, stay_pen, skip_pen, code);
            float e = erow[j0] + ls;
            const float ex = p0 - local_pen;
            bool fresh = false;
            if (VIT) { if (ex > e) { e = ex; fresh = true; } }
            else e = sh_lse(e, ex);
            if (valid) { c[j] = v; erow[j] = e; }
            if (want_tb) {
                const unsigned long long b0 = __ballot(valid && (code & 1)), b1 = __ballot(valid && (code & 2)), be = __ballot(valid && fresh);
                const int g = ch * (SH_MAP_NTH / 64) + wv;   /* the 64-cell group */
                if ((tid & 63) == 0 && 4 * g < W) {
                    uint4 w4;
                    w4.x = sh_spread16((unsigned)b0) | (sh_spread16((unsigned)b1) << 1);
                    w4.y = sh_spread16((unsigned)(b0 >> 16)) | (sh_spread16((unsigned)(b1 >> 16)) << 1);
                    w4.z = sh_spread16((unsigned)(b0 >> 32)) | (sh_spread16((unsigned)(b1 >> 32)) << 1);
                    w4.w = sh_spread16((unsigned)(b0 >> 48)) | (sh_spread16((unsigned)(b1 >> 48)) << 1);
                    *(uint4 *)(tbw + (long long)t * W + 4 * g) = w4;
                    *(uint2 *)(tbe + (long long)t * (W / 2) + 2 * g) = make_uint2((unsigned)be, (unsigned)(be >> 32));
                }
            }
        }
        start = start + ls;
        {
            float *const coln = col0 + ((t + 1) & 1) * NRP;  /* read last in block t - 1, a barrier ago */
#pragma unroll
            for (int k = 0; k < SH_MAPL_PIECES; k++) {
                const float4 f = cl.fin(q[k], sumn);
                if (tid + k * SH_MAP_NTH < NP) *(float4 *)(coln + 4 * pq[k]) = f;
            }
        }
        __syncthreads();
    }
    /* the window's end (res is free: nothing else lives there) */
    const float *const f = (NB & 1) ? buf1 : buf0;
    float x = -SH_MAP_BIG, y = -SH_MAP_BIG;
    int kx = 0x7fffffff, ky = 0x7fffffff;
    for (int j = tid; j < NC; j += SH_MAP_NTH) {
        const float cv = f[j], ev = erow[j];
        if (VIT) {
            if (cv > x || kx == 0x7fffffff) { x = cv; kx = j; }
            if (ev > y || ky == 0x7fffffff) { y = ev; ky = j; }
        } else {
            x = sh_lse(x, cv);
            y = sh_lse(y, ev);
        }
    }
    sh_map_local_reduce<VIT>(x, kx, res, tid);
    sh_map_local_reduce<VIT>(y, ky, res + 8, tid);
    if (tid == 0) {
        a.score[blockIdx.x] = VIT ? fmaxf(x, y) : sh_lse(x, y);
        if (VIT && a.final_state) a.final_state[blockIdx.x] = (x > y) ? make_int2(c0 + kx, 0) : make_int2(c0 + ky, 1);
    }
}

/* one thread per read: path[blk], blk = 0 .. nblock - 1, from the end state and the move codes; lohi[i] = (first, last) */
__global__ __launch_bounds__(64) void k_map_local_walk(const ShMapLocalWin *__restrict__ rd, int n, const unsigned *__restrict__ tb,
                                                       const int2 *__restrict__ final_state, const long long *__restrict__ path_off,
                                                       int *__restrict__ path, int2 *__restrict__ lohi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShMapLocalWin r = rd[i];
    if (!r.ok || r.tb < 0 || path_off[i] < 0) return;
    const int2 fs = final_state[i];
    const int NB = r.nblock, NC = r.ncell, c0 = r.first, W = sh_map_local_words(NC);
    const unsigned *w = tb + r.tb, *we = w + (long long)NB * W;
    int *out = path + path_off[i];
    int j = min(max(fs.x - c0, 0), NC - 1);
    int st = fs.y ? 1 : 0;                               /* 0: the cell j, 1: its E, 2: START */
    int lo = 0x7fffffff, hi = -1;
    for (int blk = NB - 1; blk >= 0; blk--) {
        out[blk] = st == 0 ? c0 + j : -1;
        if (st == 0) { lo = min(lo, c0 + j); hi = max(hi, c0 + j); }
        if (st == 1) {
            if ((we[(long long)blk * (W / 2) + (j >> 5)] >> (j & 31)) & 1u) st = 0;
        } else if (st == 0) {
            const int code = (int)((w[(long long)blk * W + (j >> 4)] >> (2 * (j & 15))) & 3u);
            if (code == 3) st = 2;
            else j = max(j - code, 0);                   /* (a path never leaves its window; never index below it) */
        }
    }
    lohi[i] = make_int2(lo == 0x7fffffff ? -1 : lo, hi + 1);
}

#endif /* SH_MAP_LOCAL_H */
