/* sh_squig_local.h -- a raw signal mapped INTO a longer reference squiggle: where in the reference the signal lies, with what score
 * and along what path.  The reference has no such function; the definition is squiggle_match_viterbi / _forward (decode.c:1016-1401;
 * k_squig, sh_squig.h) with the squiggle side made local, as k_map_local (sh_map_local.h) does for the block-based mapping.
 *
 * States: START, the positions 0 .. L - 1, the back states 0 .. L - 2 (back state k is entered from position k + 1, emits with
 * position k's parameters and leaves to position k + 1, as in sh_squig.h) and one END accumulator E[pos] per position.  Before
 * sample 0 START = 0 and everything else -SH_MAP_BIG.  Sample t, previous row p (positions) and pb (back states) to c and cb, the
 * tables of sh_squiggle_tables over the whole reference (move[0 .. L + 1], stay[0 .. L + 1]; entry 0 START's, L + 1 END's), all
 * comparisons strict > in this order:
 *   c[pos]   = p[pos] + stay[pos + 1], then step p[pos - 1] + move[pos] (pos >= 1), skip (p[pos - 2] + move[pos - 1]) - skip_pen
 *              (pos >= 2), from START p[START] + move[0] -- for EVERY pos and without a distance term --, from back
 *              pb[pos - 1] + half (pos >= 1).  START feeds positions through this move only: no step or skip out of START.
 *   cb[k]    = pb[k] + half, then p[k + 1] + back_pen (k <= L - 2)
 *   E'[pos]  = E[pos] + stay[L + 1], then p[pos] + move[pos + 1]: any position may leave, without a distance term
 * Afterwards sq_emit is added to c and cb, and local_pen is subtracted from START (= (p[START] + stay[0]) - local_pen) and from
 * every E.  End: x the first maximum of c[pos], y the first maximum of E[pos], pos ascending; the score fmaxf(x, y); the path ends in
 * the position cell iff x > y.  START and the back states are no end states.  Forward: sh_lse in place of every max.
 * Where the two definitions coincide the operations are k_squig's, one for one, under the same -ffp-contract=off.
 *
 * Windows.  A path enters the reference from START exactly once, at p0, advances at most 2 positions per sample and reaches at most
 * one cell to the left of p0 (back state p0 - 1).  Window w of stride s OWNS the paths with p0 in [w s, min((w + 1) s, L)): only
 * those cells take the START move.  It holds the cells [max(w s - 1, 0), min(w s + s - 1 + 2 (NS - 1), L - 1)]; a cell outside the
 * window reads as -SH_MAP_BIG.  Every path is owned by exactly one window and lies inside it, and its score is the same chain of
 * float additions wherever it is computed: the Viterbi score is bit-identical for every stride, one window included.  The host takes
 * the highest window (the lowest on a tie), or sh_lse over the windows in their order.  The cut is host arithmetic:
 * scrappie_hip_squiggle_local_plan (sh_host.c).
 *
 * Work split: one workgroup of SH_SQ_NTH threads per (read, window), cell j of the window (a position and its back state: they share
 * the emission) on thread j % SH_SQ_NTH; two ping-pong rows of (positions | back states) and one barrier per sample, the next
 * sample asked for before it; E is a third row that only a cell's own thread touches; START is the same chain of additions in
 * every thread's register.  Every load of the sample loop is unconditional: a lane past the window's last cell reads that cell, a
 * neighbour outside the window reads the cell at its edge, and a select puts -SH_MAP_BIG in its place.
 *
 * Homes.  LDS: the head (the end reduction's 16 words), the rows (4 ncell), E (ncell) and the window's slice of the tables -- loc,
 * scale, logsc, stay[pos + 1] (ncell each) and move[first - 1 .. first + ncell] (ncell + 2) -- in LDS: (16 + 10 ncell + 2) words,
 * while that fits SH_SQ_LDS: 1636 cells at most.  A window holds at least 2 (NS - 1) + 1 cells, so the LDS home reaches reads of up to
 * 818 samples (fewer with a stride that owns anything worth owning); longer reads, and short reads with a wide stride, keep
 * the five rows in device scratch (5 ncell floats, rounded to whole 16-byte pieces) and read the tables where the host put them, as
 * k_squig does.  Two instantiations, two launches, never a pointer that chooses at run time.
 *
 * End of a window: sh_map_local_reduce (sh_map_local.h), once over c and once over E: every thread scans its cells in order, six
 * __shfl_xor steps inside the wave, the four waves through LDS; Viterbi carries (score, cell) and takes the lower cell on equal
 * scores -- the first maximum whatever the order.
 *
 * Traceback (the second pass, on a read's best window alone): k_squig's four ballot planes per group of 64 cells (3 bits of the
 * position's move -- 0 stay, 1 step, 2 skip, 3 from START, 4 from back -- and 1 for the back state: entered from the position),
 * indexed by the cell IN the window, W = 8 ceil(ncell / 64) words per sample; behind all of them a fifth plane, "E took the fresh
 * value this sample", W / 4 words per sample.  Whole words per wave, plain vector stores by lane 0.  k_squig_local_walk, one thread
 * per read: the path (positions in the reference's coordinates, -1 in START and END, back states as their position), first -- the
 * lowest position on the path, which only the walk knows: an excursion through back state p0 - 1 dips below the entry -- and last,
 * the end cell's position + 1 (position states only move right). */
#ifndef SH_SQUIG_LOCAL_H
#define SH_SQUIG_LOCAL_H

#include "sh_map_local.h"   /* sh_map_local_reduce */
#include "sh_squig.h"       /* sq_emit, sh_squig_words, SH_SQ_* */

#define SH_SQL_HEAD 16          /* words in front of the rows: the waves' results of the two end reductions */

struct ShSquigLocalWin {
    long long sig;      /* float offset of the read's first sample */
    long long tab;      /* float offset of the reference's tables: loc[npos], scale[npos], logsc[npos], move_pen[npos + 2], stay_pen[npos + 2] */
    long long tb;       /* first traceback word (multiple of 4); -1: no traceback */
    long long scr;      /* float offset of the five rows in device scratch; -1: in LDS */
    int nsample, npos;
    int first;          /* the window's first cell (a position in the reference) */
    int ncell;          /* its cells: first .. first + ncell - 1 < npos */
    int own0;           /* the first cell IN the window that it owns as an entry position (0, or 1 behind the cell kept for the back state) */
    int own;            /* how many it owns: own0 .. own0 + own - 1 */
    int ok;             /* 0: nothing to do */
    int pad_;
};

struct ShSquigLocalArgs {
    const ShSquigLocalWin *rd;
    const float *sig;
    const float *tab;
    unsigned *tb;
    float *scr;
    float *score;               /* [window] */
    int2 *final_state;          /* [window] Viterbi: (the end position, 1: the path ends in its E, 0: in the cell) */
    float move_back_pen;        /* logf(prob_back) */
    float half_pen;             /* logf(0.5f) */
    float local_pen, skip_pen, minscore;
};

template <bool VIT, bool LDS>
__global__ __launch_bounds__(SH_SQ_NTH) void k_squig_local(ShSquigLocalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_sql_lds[];
    const ShSquigLocalWin r = a.rd[blockIdx.x];
    if (!r.ok) return;
    const int tid = threadIdx.x, L = r.npos, NS = r.nsample, NC = r.ncell, c0 = r.first;
    float *const res = sh_sql_lds;                            /* [SH_SQL_HEAD] */
    float *const buf0 = LDS ? sh_sql_lds + SH_SQL_HEAD : a.scr + r.scr;
    float *const buf1 = buf0 + 2 * NC;
    float *const erow = buf1 + 2 * NC;
    const float *const gtab = a.tab + r.tab;
    float *const ltab = sh_sql_lds + SH_SQL_HEAD + 5 * NC;    /* loc | scale | logsc | move[c0 - 1 ..] (NC + 2) | stay[c0 + 1 ..] */
    if (LDS) {
        for (int j = tid; j < NC; j += SH_SQ_NTH) {
            ltab[j] = gtab[c0 + j];
            ltab[NC + j] = gtab[L + c0 + j];
            ltab[2 * NC + j] = gtab[2 * L + c0 + j];
            ltab[4 * NC + 2 + j] = gtab[4 * L + 2 + c0 + j + 1];
        }
        for (int i = tid; i < NC + 2; i += SH_SQ_NTH) ltab[3 * NC + i] = gtab[3 * L + max(c0 - 1 + i, 0)];      /* (c0 + NC <= L: move[L] exists) */
    }
    /* by the cell in the window: loc[j], scale[j], logsc[j]; mv[j + d] = move_pen[c0 + j + d], d = -1, 0, 1; st[j] = stay_pen[c0 + j + 1].  (Scratch home,
     * c0 = 0: mv[-1] is the table in front of move_pen; it is read for cell 0 and never used: a skip needs pos >= 2.) */
    const float *const loc = LDS ? (const float *)ltab : gtab + c0;
    const float *const scale = LDS ? (const float *)ltab + NC : gtab + L + c0;
    const float *const logsc = LDS ? (const float *)ltab + 2 * NC : gtab + 2 * L + c0;
    const float *const mv = LDS ? (const float *)ltab + 3 * NC + 1 : gtab + 3 * L + c0;
    const float *const st = LDS ? (const float *)ltab + 4 * NC + 2 : gtab + 4 * L + 2 + c0 + 1;
    const float move0 = gtab[3 * L], stay0 = gtab[4 * L + 2], stayE = gtab[4 * L + 2 + L + 1];
    for (int j = tid; j < 2 * NC; j += SH_SQ_NTH) { buf0[j] = -SH_MAP_BIG; buf1[j] = -SH_MAP_BIG; }
    for (int j = tid; j < NC; j += SH_SQ_NTH) erow[j] = -SH_MAP_BIG;
    const float *const sig = a.sig + r.sig;
    const float local_pen = a.local_pen, skip_pen = a.skip_pen, minscore = a.minscore, back_pen = a.move_back_pen, half_pen = a.half_pen;
    const bool want_tb = VIT && r.tb >= 0;
    const long long W = sh_squig_words(NC);
    unsigned *const tbw = want_tb ? a.tb + r.tb : nullptr;
    unsigned *const tbe = want_tb ? tbw + (long long)NS * W : nullptr;
    const int nch = (NC + SH_SQ_NTH - 1) / SH_SQ_NTH, ngrp = (NC + 63) / 64;
    const int wv = tid >> 6, ln = tid & 63;
    const int own_lo = r.own0, own_hi = r.own0 + r.own;
    float start = 0.0f;                                      /* START before sample t: the same in every thread */
    float x = sig[0];
    __syncthreads();
    for (int t = 0; t < NS; t++) {
        const float *const p = (t & 1) ? buf1 : buf0, *const pb = p + NC;
        float *const c = (t & 1) ? buf0 : buf1, *const cb = c + NC;
        const float xn = sig[t + 1 < NS ? t + 1 : t];        /* the next sample, asked for before the barrier */
        const float from_start = start + move0;
        for (int ch = 0; ch < nch; ch++) {
            const int j = ch * SH_SQ_NTH + tid;
            const bool valid = j < NC;
            const int j0 = min(j, NC - 1), j1 = max(j0 - 1, 0), j2 = max(j0 - 2, 0), jr = min(j0 + 1, NC - 1), pos = c0 + j0;
            const float pv = p[j0], l1 = p[j1], l2 = p[j2], rr = p[jr], bv = pb[j0], bl = pb[j1], ev = erow[j0];
            const float p1 = j0 >= 1 ? l1 : -SH_MAP_BIG, p2 = j0 >= 2 ? l2 : -SH_MAP_BIG;       /* outside the window: no owned path */
            const float pr = j0 + 1 < NC ? rr : -SH_MAP_BIG, b1 = j0 >= 1 ? bl : -SH_MAP_BIG;
            const float em = sq_emit(x, loc[j0], scale[j0], logsc[j0], minscore);
            const bool mine = j0 >= own_lo && j0 < own_hi;
            float v = pv + st[j0];
            const float s1 = p1 + mv[j0];
            const float s2 = (p2 + mv[j0 - 1]) - skip_pen;
            const float fb = b1 + half_pen;
            float bk = bv + half_pen;
            const float mb = pr + back_pen;
            float e = ev + stayE;
            const float ex = pv + mv[j0 + 1];
            int code = 0, bbit = 0;
            bool fresh = false;
            if (VIT) {
                if (pos >= 1 && s1 > v) { v = s1; code = 1; }
                if (pos >= 2 && s2 > v) { v = s2; code = 2; }
                if (mine && from_start > v) { v = from_start; code = 3; }
                if (pos >= 1 && fb > v) { v = fb; code = 4; }
                if (pos <= L - 2 && mb > bk) { bk = mb; bbit = 1; }
                if (ex > e) { e = ex; fresh = true; }
            } else {
                if (pos >= 1) v = sh_lse(v, s1);
                if (pos >= 2) v = sh_lse(v, s2);
                if (mine) v = sh_lse(v, from_start);
                if (pos >= 1) v = sh_lse(v, fb);
                if (pos <= L - 2) bk = sh_lse(bk, mb);
                e = sh_lse(e, ex);
            }
            if (valid) { c[j] = v + em; cb[j] = bk + em; erow[j] = e - local_pen; }
            if (want_tb) {
                const unsigned long long b0 = __ballot(valid && (code & 1)), b1_ = __ballot(valid && (code & 2)), b2 = __ballot(valid && (code & 4)),
                                         b3 = __ballot(valid && bbit), be = __ballot(valid && fresh);
                const int g = ch * (SH_SQ_NTH / 64) + wv;
                if (ln == 0 && g < ngrp) {
                    uint4 *dst = (uint4 *)(tbw + (long long)t * W + (long long)g * 8);
                    dst[0] = make_uint4((unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1_, (unsigned)(b1_ >> 32));
                    dst[1] = make_uint4((unsigned)b2, (unsigned)(b2 >> 32), (unsigned)b3, (unsigned)(b3 >> 32));
                    *(uint2 *)(tbe + (long long)t * (W / 4) + (long long)g * 2) = make_uint2((unsigned)be, (unsigned)(be >> 32));
                }
            }
        }
        start = (start + stay0) - local_pen;
        x = xn;
        __syncthreads();
    }
    /* the window's end */
    const float *const f = (NS & 1) ? buf1 : buf0;
    float xs = -SH_MAP_BIG, ys = -SH_MAP_BIG;
    int kx = 0x7fffffff, ky = 0x7fffffff;
    for (int j = tid; j < NC; j += SH_SQ_NTH) {
        const float cv = f[j], ev = erow[j];
        if (VIT) {
            if (cv > xs || kx == 0x7fffffff) { xs = cv; kx = j; }
            if (ev > ys || ky == 0x7fffffff) { ys = ev; ky = j; }
        } else {
            xs = sh_lse(xs, cv);
            ys = sh_lse(ys, ev);
        }
    }
    sh_map_local_reduce<VIT>(xs, kx, res, tid);
    sh_map_local_reduce<VIT>(ys, ky, res + 8, tid);
    if (tid == 0) {
        a.score[blockIdx.x] = VIT ? fmaxf(xs, ys) : sh_lse(xs, ys);
        if (VIT && a.final_state) a.final_state[blockIdx.x] = (xs > ys) ? make_int2(c0 + kx, 0) : make_int2(c0 + ky, 1);
    }
}

/* one thread per read: path[t], t = 0 .. nsample - 1, from the end state and the planes; lohi[i] = (first, last) */
__global__ __launch_bounds__(64) void k_squig_local_walk(const ShSquigLocalWin *__restrict__ rd, int n, const unsigned *__restrict__ tb,
                                                         const int2 *__restrict__ final_state, const long long *__restrict__ path_off,
                                                         int *__restrict__ path, int2 *__restrict__ lohi) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShSquigLocalWin r = rd[i];
    if (!r.ok || r.tb < 0 || path_off[i] < 0) return;
    const int2 fs = final_state[i];
    const int NS = r.nsample, NC = r.ncell, c0 = r.first;
    const long long W = sh_squig_words(NC);
    const unsigned *w = tb + r.tb, *we = w + (long long)NS * W;
    int *out = path + path_off[i];
    int j = min(max(fs.x - c0, 0), NC - 1);
    int st = fs.y ? 1 : 0;                               /* 0: the position of cell j, 1: its E, 2: START, 3: its back state */
    int lo = 0x7fffffff;
    for (int t = NS - 1; t >= 0; t--) {
        const bool on = st == 0 || st == 3;
        out[t] = on ? c0 + j : -1;
        if (on) lo = min(lo, c0 + j);
        const int wd = (j >> 6) * 8 + ((j & 63) >> 5), sh = j & 31;
        if (st == 1) {
            if ((we[(long long)t * (W / 4) + (j >> 6) * 2 + ((j & 63) >> 5)] >> sh) & 1u) st = 0;
        } else if (st == 0) {
            const unsigned *g = w + (long long)t * W + wd;
            const int code = (int)(((g[0] >> sh) & 1u) | (((g[2] >> sh) & 1u) << 1) | (((g[4] >> sh) & 1u) << 2));
            if (code == 3) st = 2;
            else if (code == 4) { st = 3; j = max(j - 1, 0); }
            else j = max(j - code, 0);                   /* (a path never leaves its window; never index below it) */
        } else if (st == 3) {
            if ((w[(long long)t * W + wd + 6] >> sh) & 1u) { st = 0; j = min(j + 1, NC - 1); }
        }
    }
    lohi[i] = make_int2(lo == 0x7fffffff ? -1 : lo, fs.x + 1);
}

#endif /* SH_SQUIG_LOCAL_H */
