/* sh_map_edits.h -- part of sh_kernels.h (included from there, behind sh_map_local.h): EVERY single-base edit of a sequence scored against
 * a read of a transducer model in one pass -- 4 L substitutions (the L that change nothing among them), L deletions, 4 (L + 1) insertions --
 * each the score map_to_sequence_viterbi / _forward (k_map, sh_map.h) give for the k-mer states of the edited sequence.  Scores only; unbanded, or
 * (the BAND instantiations, at the end of this comment) inside a band of map_to_sequence_*_banded's kind.
 *
 * The lattice is k_map's: states s[q] = kmer(seq[q .. q + k)), q = 0 .. n - 1, n = L - k + 1; START, END; stay, step, skip.  Entries
 * t = 0 .. NB, block t leads from entry t to entry t + 1.  lps the block's stay entry, ls = mx(-local_pen, lps).
 *     F[t][q], FS[t]    k_map's cells and START, kept for every entry;
 *     G[t][q]           the best (forward: the sum over) continuations from cell q at entry t to the end, GE[t] END's from entry t:
 *         GE[NB] = 0, GE[t] = GE[t + 1] + ls_t;  G[NB][n - 1] = 0, everything else -SH_MAP_BIG;
 *         G[t][q] = (lps - stay_pen) + G[t + 1][q], then mx with lp[t][s[q + 1]] + G[t + 1][q + 1] (q + 1 < n), with
 *         (lp[t][s[q + 2]] - skip_pen) + G[t + 1][q + 2] (q + 2 < n), with -local_pen + GE[t + 1] (q == n - 1).
 * mx(a, b): b if b > a else a (Viterbi), sh_lse(a, b) (forward).  An edit at base i keeps the first A = max(i - k + 1, 0) states, puts M <= k
 * new states mid[0..M) behind them -- the k-mers that hold the new base, or that close over the deleted one -- and continues with the suffix
 * s[j0 ..] of Bn = n - j0 states; J = A + M is the suffix's first index in the edited sequence.  The edit runs its own M columns down the
 * entries (k_map's cell rule at index A + m, reading the columns to their left: its own, or the prefix's F) and joins the suffix where a path
 * reaches it for the FIRST time: at block t in its first state (Y0: step from J - 1, skip from J - 2, START where J == 0; no stay) or, by a
 * skip from J - 1, in its second (Y1); from there on the path lies in cells the edit does not touch, G.  Without a suffix END's own chain and
 * k_map's end rule close on the last column.  include/scrappie_hip.h states the whole definition; tests/test_map_edits_cpu.py restates it.
 * The build has -ffp-contract=off; the Viterbi form holds additions and compares only.
 *
 * k_map_edits_rows<VIT, TILED, BACK>: k_map's unbanded LDS form -- one workgroup of SH_MAP_NTH threads per read, cell q on thread
 * q % SH_MAP_NTH, two ping-pong rows of n + 2 floats in LDS beside the state codes, one barrier per block, a cell's posterior entries
 * gathered through ShMapPost<TILED> -- that also stores every completed row to device memory as [entry][cell] floats, `pitch` apart.
 * !BACK: blocks ascending through sh_map_cell<VIT>, so the rows and `base` are k_map's bits by construction; slot n of a row holds FS[t]
 * (LDS and device memory alike), END is thread 0's.  BACK: blocks descending, the recursion above, GE a chain in every thread's registers;
 * slot n takes the stores of threads without a cell.  The row stores are unconditional plain vector stores.  LDS is the only home of the
 * rows: n is at most what k_map's LDS home holds.
 *
 * k_map_edits<VIT, TILED>: one thread per base position i = 0 .. L, consecutive lanes on consecutive i, SH_MAP_NTH positions per workgroup
 * (grid: read x chunk of positions).  The thread walks the blocks serially.  In registers: the middle columns of its nine edits (4 x SH_ME_K
 * for sub, as many for ins, SH_ME_K - 1 for del; slot m is index A + m, slots from M on idle), updated in place, m descending, and nine
 * running scores; the codes of the new states as a code with base A in the new base's digit and that digit's weight.  Per block it loads
 * F[t][A - 1], F[t][A - 2], FS[t] and G[t + 1][i .. i + 2] (coalesced, indices clamped, SH_ME_D blocks ahead).  Posterior entries come
 * from the block's whole column in LDS, staged as k_map_local stages it (ShMapLocalCol<TILED>: every entry finalised once by the fin_post
 * call k_map makes), SH_ME_CH blocks per barrier, double-buffered, the next chunk already in registers.  Every LDS and vector-memory operation
 * of the block loop is unconditional: clamped indices, selects, no lane conditions.
 * Results per read at res: sub [L][4], ins [L + 1][4], del [L] (in this order: the float4 stores stay 16-byte aligned); a score below
 * -SH_MAP_BIG / 2: no admissible path (the host answers NAN).  All stores are plain vector stores.
 *
 * BAND = true (ShMapEditsBandRead, below): F and G hold -SH_MAP_BIG outside the band of their entry and an entry's row holds its band's cells alone.
 * The rows kernel has ONE block loop for both forms -- per entry the cells from the 64-cell group of low on and at least one thread without a
 * cell, the previous row read under the previous entry's band (forward: sh_map_cell on a ShMapEditsRow, whose reads of the cells to the left and
 * of START sit under its position tests, as in k_map) -- whose bounds without a band are the
 * constants 0 and n; BAND decides the bounds, the first chunk's base and the row index of the global store alone.  k_map_edits: a few
 * `if constexpr` lines. */
#ifndef SH_MAP_EDITS_H
#define SH_MAP_EDITS_H

#include "sh_map_local.h"   /* sh_map.h: SH_MAP_NTH, SH_MAP_BIG, sh_lse, ShMapPost, sh_map_cell; ShMapLocalCol, SH_MAPL_PIECES */

#define SH_ME_K 5                 /* middle columns an edit may have: the longest k-mer */
#define SH_ME_CH 4                /* blocks of posterior columns staged in LDS per barrier of k_map_edits */
#define SH_ME_D 4                 /* blocks of row values in flight per thread of k_map_edits (divides SH_ME_CH) */

struct ShMapEditsRead {
    long long post;     /* dense: float offset of the read's row 0; tiled: the read's first column block */
    long long seq;      /* offset of the read's n state codes in seq[] */
    long long bases;    /* offset of its L base codes in seq[] */
    long long rows;     /* float offset of F in rows[]; G lies (nblock + 1) * pitch floats behind it */
    long long res;      /* float offset of the read's results in res[] (a multiple of 4) */
    int nblock, nbase;
    int lane;           /* tiled: the read's lane in its tile (0..15) */
    int pitch;          /* floats from one entry's row to the next (>= n + 1) */
};

template <class Rec> struct ShMapEditsArgsT {
    const Rec *rd;
    const float *post;          /* dense posterior */
    const float *E, *sums;      /* tiled posterior */
    long long pstride;          /* dense: floats per row (a multiple of 4, at least 4 ceil(nr / 4)) */
    int nr;                     /* states, stay included: 4^k + 1 */
    int nchunk;                 /* tiled: chunks of 16 states per column block */
    int k;                      /* bases per state, 1 .. SH_ME_K */
    float min_prob;             /* tiled: fin_post's floor */
    float stay_pen, skip_pen, local_pen;
    const int *seq;
    float *rows;
    float *res;
    float *base;                /* [read] */
};
using ShMapEditsArgs = ShMapEditsArgsT<ShMapEditsRead>;

/* A read in a band: low and high of nblock int32 each, as map_to_sequence_*_banded take them (in seq[] behind the codes): cell q of entry t + 1 is
 * admissible iff low[t] <= q < high[t]; entry 0 has no cells.  An entry's row holds its band's cells alone, cell q of entry t + 1 at float q - low[t],
 * and the slot at pitch - 1 holds FS (forward) or takes the stores of threads without a cell (backward): pitch is the widest entry's cells and that
 * slot rounded up to 16 (scrappie_hip_map_edits_band_pitch). */
struct ShMapEditsBandRead : ShMapEditsRead {
    long long band;     /* offset in seq[] of low; high the next nblock */
};
struct ShMapEditsBandArgs : ShMapEditsArgsT<ShMapEditsBandRead> {
    int width;          /* host only: the positions per workgroup of k_map_edits this launch takes (64 or 256) */
};
template <bool BAND> using ShMapEditsArgsOf = std::conditional_t<BAND, ShMapEditsBandArgs, ShMapEditsArgs>;
/* what the kernels take of the caller, from one form's arguments to the other's: the one place the fields are copied (the launch sets the rest) */
template <class To, class From> static To sh_map_edits_args_as(const From &u) {
    To a{};
    a.post = u.post; a.E = u.E; a.sums = u.sums; a.pstride = u.pstride; a.nr = u.nr; a.nchunk = u.nchunk; a.k = u.k; a.min_prob = u.min_prob;
    a.stay_pen = u.stay_pen; a.skip_pen = u.skip_pen; a.local_pen = u.local_pen;
    return a;
}

/* the band of entry e of a read of NB blocks: [lo, hi); entry 0 has none */
__device__ __forceinline__ void sh_me_band(const int *blo, int NB, int e, int &lo, int &hi) {
    const int j = min(max(e - 1, 0), NB - 1);
    lo = blo[j];
    const int h = blo[NB + j];
    hi = e >= 1 ? h : lo;
}

template <bool VIT> __device__ __forceinline__ float sh_me_mx(float a, float b) { return VIT ? (b > a ? b : a) : sh_lse(a, b); }
/* mx(a, b) where on, else a: a select (Viterbi); forward, sh_lse with an operand so far below that it adds exactly nothing */
template <bool VIT> __device__ __forceinline__ float sh_me_mx_if(bool on, float a, float b) {
    return VIT ? ((on && b > a) ? b : a) : sh_lse(a, on ? b : -4.0f * SH_MAP_BIG);
}

/* a row of n cells under the band [lo, hi) of its entry, as sh_map_cell reads one: a cell outside the band is -SH_MAP_BIG; the slots from n on
 * (START, END) and, without a band, everything as they stand */
template <bool BAND> struct ShMapEditsRow {
    const float *p;
    int lo, hi, n;
    __device__ __forceinline__ float operator[](int x) const {
        const float l = p[x];
        return (!BAND || x >= n || (x >= lo && x < hi)) ? l : -SH_MAP_BIG;
    }
};

template <bool VIT, bool TILED, bool BACK, bool BAND = false>
__global__ __launch_bounds__(SH_MAP_NTH) void k_map_edits_rows(ShMapEditsArgsOf<BAND> a) {
    extern __shared__ __attribute__((aligned(16))) float sh_me_lds[];
    const auto r = a.rd[blockIdx.x];
    const int tid = threadIdx.x, n = r.nbase - a.k + 1, NB = r.nblock, RW = n + 2, START = n, END = n + 1, STAY = a.nr - 1;
    const long long P = r.pitch;
    const float stay_pen = a.stay_pen, skip_pen = a.skip_pen, local_pen = a.local_pen;
    float *const buf0 = sh_me_lds;
    float *const buf1 = buf0 + RW;
    int *const sq = (int *)(sh_me_lds + 2 * RW);
    for (int i = tid; i < n; i += SH_MAP_NTH) sq[i] = a.seq[r.seq + i];
    float *const grow = a.rows + r.rows + (BACK ? (long long)(NB + 1) * P : 0);
    /* BAND: the band of the entry a step reads (lo_p, hi_p) and of the one it completes (lo_c, hi_c) */
    const int *blo = nullptr;
    int lo_p = 0, hi_p = n, lo_c = 0, hi_c = n;
    if constexpr (BAND) {
        blo = a.seq + r.band;
        sh_me_band(blo, NB, BACK ? NB : 0, lo_p, hi_p);
        sh_me_band(blo, NB, BACK ? NB - 1 : 1, lo_c, hi_c);
        float *const g0 = grow + (BACK ? (long long)NB * P : 0);
        for (int i = tid; i < RW; i += SH_MAP_NTH) {         /* the first row: entry 0 (no cells), or entry NB (cell n - 1 where it is admissible) */
            buf0[i] = BACK ? ((i == n - 1 && i >= lo_p && i < hi_p) ? 0.0f : -SH_MAP_BIG) : (i == START ? 0.0f : -SH_MAP_BIG);
            buf1[i] = -SH_MAP_BIG;
        }
        for (int i = tid; i < (int)P; i += SH_MAP_NTH)       /* (the slot at P - 1: FS[0] = 0; backward nothing reads it) */
            g0[i] = BACK ? ((lo_p + i == n - 1 && lo_p + i < hi_p) ? 0.0f : -SH_MAP_BIG) : (i == (int)P - 1 ? 0.0f : -SH_MAP_BIG);
    } else {
        float *const g0 = grow + (BACK ? (long long)NB * P : 0);
        for (int i = tid; i < RW; i += SH_MAP_NTH) {         /* the first row: entry 0, or entry NB */
            const float v = BACK ? (i == n - 1 ? 0.0f : -SH_MAP_BIG) : (i == START ? 0.0f : -SH_MAP_BIG);
            buf0[i] = v;
            buf1[i] = -SH_MAP_BIG;
            g0[min(i, n)] = i <= n ? v : (BACK ? -SH_MAP_BIG : 0.0f);      /* (slot n: FS[0] = 0; backward nothing reads it) */
        }
    }
    ShMapArgs ma{};
    ma.post = a.post; ma.E = a.E; ma.sums = a.sums; ma.pstride = a.pstride; ma.nr = a.nr; ma.nchunk = a.nchunk; ma.min_prob = a.min_prob;
    ShMapRead mr{};
    mr.post = r.post; mr.lane = r.lane;
    ShMapPost<TILED> lp;
    float chain = 0.0f;                                      /* FS[t] going forward, GE[t + 1] going backward: the same in every thread */
    __syncthreads();
    for (int step = 0; step < NB; step++) {
        const int t = BACK ? NB - 1 - step : step;
        const float *const p = (step & 1) ? buf1 : buf0;
        float *const c = (step & 1) ? buf0 : buf1;
        float *const g = grow + (long long)(BACK ? t : t + 1) * P;      /* the entry this step completes */
        lp.block(ma, mr, t);
        const float lps = lp(STAY);
        const float ls = VIT ? fmaxf(-local_pen, lps) : sh_lse(-local_pen, lps);
        /* the band's cells alone, from the 64-cell group of lo_c on, and at least one thread without a cell; without a band the bounds are 0 and n,
         * constants: cells 0 .. n - 1 and slot n */
        int lo_n = 0, hi_n = n;
        if constexpr (BAND) sh_me_band(blo, NB, BACK ? max(t - 1, 0) : min(t + 2, NB), lo_n, hi_n);      /* asked for before the barrier */
        const int base = lo_c & ~63;
        const int nchb = (hi_c - base + SH_MAP_NTH) / SH_MAP_NTH;
        auto in_p = [&](int x) { return !BAND || (x >= lo_p && x < hi_p); };      /* cell x of the entry read */
        for (int ch = 0; ch < nchb; ch++) {
            const int pos = base + ch * SH_MAP_NTH + tid, q = min(pos, n - 1);
            const bool valid = pos >= lo_c && pos < hi_c;
            float v;
            if (!BACK) {                                     /* k_map's unbanded cell on the masked row */
                int code;
                const float cell = sh_map_cell<VIT>(ShMapEditsRow<BAND>{p, lo_p, hi_p, n}, q, START, q, lp(sq[q]), lps, stay_pen, skip_pen, code);
                v = valid ? cell : chain + ls;               /* the slot: FS[t + 1] */
            } else {
                const int q1 = min(q + 1, n - 1), q2 = min(q + 2, n - 1);
                const float le1 = lp(sq[q1]), le2 = lp(sq[q2]);
                const float l0 = p[q], l1 = p[q1], l2 = p[q2];
                const float g0 = in_p(q) ? l0 : -SH_MAP_BIG, g1 = in_p(q1) ? l1 : -SH_MAP_BIG, g2 = in_p(q2) ? l2 : -SH_MAP_BIG;
                v = (lps - stay_pen) + g0;
                v = sh_me_mx_if<VIT>(q + 1 < n, v, le1 + g1);
                v = sh_me_mx_if<VIT>(q + 2 < n, v, (le2 - skip_pen) + g2);
                v = sh_me_mx_if<VIT>(q == n - 1, v, -local_pen + chain);
            }
            c[valid ? pos : n] = v;
            g[!BAND ? (long long)min(pos, n) : valid ? (long long)(pos - lo_c) : P - 1] = v;      /* BAND: the row holds the band's cells; its last slot is no cell's */
        }
        if (!BACK && tid == 0) {                             /* END, as k_map keeps it, reading cell n - 1 under its band */
            float e = p[END] + ls;
            const float pl = p[n - 1];
            const float ex = (in_p(n - 1) ? pl : -SH_MAP_BIG) - local_pen;
            if (VIT) { if (ex > e) e = ex; }
            else e = sh_lse(e, ex);
            c[END] = e;
        }
        if constexpr (BAND) { lo_p = lo_c; hi_p = hi_c; lo_c = lo_n; hi_c = hi_n; }
        chain = chain + ls;
        __syncthreads();
    }
    if (!BACK && tid == 0) {
        const float *const f = (NB & 1) ? buf1 : buf0;
        const float fx = f[n - 1], y = f[END];
        const float x = (!BAND || (n - 1 >= lo_p && n - 1 < hi_p)) ? fx : -SH_MAP_BIG;      /* (BAND: entry NB's band) */
        a.base[blockIdx.x] = VIT ? fmaxf(x, y) : sh_lse(x, y);
    }
}

/* the edited sequence's base at p with code 0 for the new base; kind 0 sub, 1 del, 2 ins; sq: the L bases */
__device__ __forceinline__ int sh_me_base(int kind, int p, int i, const int *sq, int L) {
    const int src = kind == 0 ? p : kind == 1 ? (p < i ? p : p + 1) : (p < i ? p : p - 1);
    const int b = sq[min(max(src, 0), L - 1)];
    return (kind != 1 && p == i) ? 0 : b;
}

/* One edit at one block: its join with the suffix (or END's chain where it has none), then its NS middle columns X, in place.
 * fa2, fa1: the prefix's columns A - 2, A - 1 at entry t, fs START's; col: the block's posterior column; code0[m] + cw[m]: the state of slot m.
 * le0, le1, g0, g1: the posterior entries of the suffix's first two states and G[t + 1] of them. */
template <bool VIT, int NS>
__device__ __forceinline__ void sh_me_edit(float (&X)[NS], float &acc, const int (&code0)[NS], const int (&cw)[NS], int cmul, int A, int M, int J, int Bn,
                                           float fa2, float fa1, float fs, const float *col, float lps, float ls, float le0, float le1, float g0,
                                           float g1, float stay_pen, float skip_pen, float local_pen) {
    float c1 = fa1, c2 = fa2;                                /* columns J - 1 and J - 2 at entry t */
#pragma unroll
    for (int j = 1; j <= NS; j++) {
        c1 = M == j ? X[j - 1] : c1;
        c2 = M == j ? (j == 1 ? fa1 : X[j - 2 < 0 ? 0 : j - 2]) : c2;
    }
    const bool closed = Bn == 0;
    float y0 = (J == 0 ? fs : c1) + le0;
    y0 = sh_me_mx_if<VIT>(J >= 2, y0, (c2 - skip_pen) + le0);
    const float a1 = closed ? acc + ls : acc, b1 = closed ? c1 - local_pen : y0 + g0;
    acc = sh_me_mx<VIT>(a1, b1);
    acc = sh_me_mx_if<VIT>(Bn >= 2 && J >= 1, acc, ((c1 - skip_pen) + le1) + g1);
#pragma unroll
    for (int m = NS - 1; m >= 0; m--) {
        const int q = A + m;
        const float le = col[code0[m] + cmul * cw[m]];
        const float l1 = m == 0 ? fa1 : X[m - 1 < 0 ? 0 : m - 1];
        const float l2 = m == 0 ? fa2 : m == 1 ? fa1 : X[m - 2 < 0 ? 0 : m - 2];
        float v = (X[m] - stay_pen) + lps;
        v = sh_me_mx<VIT>(v, (q >= 1 ? l1 : fs) + le);       /* the step, or from START at index 0 */
        v = sh_me_mx_if<VIT>(q >= 2, v, (l2 - skip_pen) + le);
        X[m] = m < M ? v : X[m];
    }
}

/* the column J - 1 of an edit after the last block */
template <int NS> __device__ __forceinline__ float sh_me_last(const float (&X)[NS], int M, float fa1) {
    float c1 = fa1;
#pragma unroll
    for (int j = 1; j <= NS; j++) c1 = M == j ? X[j - 1] : c1;
    return c1;
}

template <bool VIT, bool TILED, bool BAND = false, int W = SH_MAP_NTH>
__global__ __launch_bounds__(W) void k_map_edits(ShMapEditsArgsOf<BAND> a) {
    extern __shared__ __attribute__((aligned(16))) float sh_me_cols[];      /* [2][SH_ME_CH][NRP] */
    constexpr int NPC = ((1 << (2 * SH_ME_K - 2)) + 1 + W - 1) / W;         /* 16-byte pieces of a column per thread: 4^SH_ME_K + 1 states at most */
    static_assert(W == SH_MAP_NTH ? NPC == SH_MAPL_PIECES : true, "a workgroup of SH_MAP_NTH stages as k_map_local does");
    const auto r = a.rd[blockIdx.x];
    const int L = r.nbase, K = a.k, n = L - K + 1, NB = r.nblock, tid = threadIdx.x;
    const int i0 = blockIdx.y * W;
    if (i0 > L) return;                                      /* (uniform) */
    const bool mine = i0 + tid <= L;
    const int i = min(i0 + tid, L);
    const int NP = (a.nr + 3) >> 2, NRP = NP * 4, STAY = a.nr - 1;
    const float stay_pen = a.stay_pen, skip_pen = a.skip_pen, local_pen = a.local_pen;
    const long long P = r.pitch;
    const float *const F = a.rows + r.rows, *const G = F + (long long)(NB + 1) * P;
    /* BAND: the workgroup walks blocks T0 .. T1 - 1 alone.  Before block T0 -- entry T0 the first whose band reaches the lowest cell a position of
     * the workgroup takes a prefix value from, max(A(i0) - 2, 0): high[T0 - 1] > it; 0 where a position enters from START (i0 < K) -- every source is
     * -SH_MAP_BIG: the middle columns and the running scores stay what they were set to.  From block T1 on -- low[T1] above the furthest cell a position
     * joins, min(i1 + 2, n - 1) -- every G is -SH_MAP_BIG and nothing joins; NB where a position closes by END's chain (i1 >= n - 1).  Both edges
     * are non-decreasing: two counts over the band. */
    const int *blo = nullptr;
    int T0 = 0, T1 = NB;
    if constexpr (BAND) {
        __shared__ int cnt[2];
        blo = a.seq + r.band;
        if (tid < 2) cnt[tid] = 0;
        __syncthreads();
        const int i1 = min(i0 + W - 1, L);
        const int cmin = max(max(i0 - K + 1, 0) - 2, 0), cmax = min(i1 + 2, n - 1);
        int below = 0, reach = 0;
        for (int t = tid; t < NB; t += W) { below += blo[NB + t] <= cmin; reach += blo[t] <= cmax; }
        if (below) atomicAdd(&cnt[0], below);
        if (reach) atomicAdd(&cnt[1], reach);
        __syncthreads();
        T0 = i0 < K ? 0 : min(cnt[0] + 1, NB);
        T1 = i1 >= n - 1 ? NB : cnt[1];
    }
    /* what the three kinds share: the prefix's states, the suffix's candidates */
    const int A = max(i - K + 1, 0);
    const float *const FA1 = F + max(A - 1, 0), *const FA2 = F + max(A - 2, 0), *const FSp = F + n;
    const float *const GA = G + min(i, n - 1), *const GB = G + min(i + 1, n - 1), *const GC = G + min(i + 2, n - 1);
    /* BAND: cell c of entry e from the matrix at m; outside the band -SH_MAP_BIG, the index clamped into the row */
    auto cell = [&](const float *m, int e, int c, int lo, int hi) {
        const float x = m[(long long)e * P + min(max(c - lo, 0), (int)P - 1)];
        return c >= lo && c < hi ? x : -SH_MAP_BIG;
    };
    const int *const st = a.seq + r.seq, *const bs = a.seq + r.bases;
    const int sA = st[min(i, n - 1)], sB = st[min(i + 1, n - 1)], sC = st[min(i + 2, n - 1)];
    /* sub and del: the suffix begins at min(i + 1, n); ins: at min(i, n) */
    const int j0s = min(i + 1, n), j0i = min(i, n);
    const int Bs = n - j0s, Bi = n - j0i;
    const int Js = j0s, Jd = j0s - 1, Ji = j0i + 1;
    const int Ms = Js - A, Md = max(Jd - A, 0), Mi = Ji - A;
    int cs[SH_ME_K], ci[SH_ME_K], cd[SH_ME_K - 1], cw[SH_ME_K], zw[SH_ME_K - 1];
#pragma unroll
    for (int m = 0; m < SH_ME_K; m++) {
        int vs = 0, vi = 0, vd = 0;
#pragma unroll
        for (int j = 0; j < SH_ME_K; j++)
            if (j < K) {
                vs = vs * 4 + sh_me_base(0, A + m + j, i, bs, L);
                vd = vd * 4 + sh_me_base(1, A + m + j, i, bs, L);
                vi = vi * 4 + sh_me_base(2, A + m + j, i, bs, L);
            }
        const int j = i - (A + m);                           /* where the new base stands in this k-mer */
        cs[m] = vs; ci[m] = vi;
        cw[m] = (j >= 0 && j < K) ? 1 << (2 * (K - 1 - j)) : 0;
        if (m < SH_ME_K - 1) { cd[m] = vd; zw[m] = 0; }
    }
    ShMapLocalArgs la{};
    la.post = a.post; la.E = a.E; la.sums = a.sums; la.pstride = a.pstride; la.nr = a.nr; la.nchunk = a.nchunk; la.min_prob = a.min_prob;
    ShMapLocalWin lw{};
    lw.post = r.post; lw.lane = r.lane;
    const ShMapLocalCol<TILED> cl(la, lw);
    int pq[NPC];
#pragma unroll
    for (int k = 0; k < NPC; k++) pq[k] = min(tid + k * W, NP - 1);
    float4 q[SH_ME_CH][NPC];
    float qs[SH_ME_CH];
    auto fetch = [&](int c) {
#pragma unroll
        for (int u = 0; u < SH_ME_CH; u++) {
            const int blk = min((BAND ? T0 : 0) + c * SH_ME_CH + u, NB - 1);
            qs[u] = cl.scale(blk);
#pragma unroll
            for (int k = 0; k < NPC; k++) q[u][k] = cl.piece(blk, pq[k]);
        }
    };
    auto stage = [&](int buf) {                              /* (a piece past the column's last is its last again: the same words twice) */
#pragma unroll
        for (int u = 0; u < SH_ME_CH; u++)
#pragma unroll
            for (int k = 0; k < NPC; k++)
                *(float4 *)(sh_me_cols + (long long)(buf * SH_ME_CH + u) * NRP + 4 * pq[k]) = cl.fin(q[u][k], qs[u]);
    };
    fetch(0);
    stage(0);
    fetch(1);
    /* block t reads the prefix's cells of entry t and the suffix's of entry t + 1 */
    float fa1[SH_ME_D], fa2[SH_ME_D], fs[SH_ME_D], gA[SH_ME_D], gB[SH_ME_D], gC[SH_ME_D];
    auto rows_of = [&](int t, int d) {
        if constexpr (BAND) {
            const int t0 = min(t, NB), t1 = min(t + 1, NB);
            int l0, h0, l1, h1;
            sh_me_band(blo, NB, t0, l0, h0);
            sh_me_band(blo, NB, t1, l1, h1);
            fa1[d] = cell(F, t0, max(A - 1, 0), l0, h0); fa2[d] = cell(F, t0, max(A - 2, 0), l0, h0); fs[d] = F[(long long)t0 * P + (P - 1)];
            gA[d] = cell(G, t1, min(i, n - 1), l1, h1); gB[d] = cell(G, t1, min(i + 1, n - 1), l1, h1); gC[d] = cell(G, t1, min(i + 2, n - 1), l1, h1);
        } else {
            const long long e0 = (long long)min(t, NB) * P, e1 = (long long)min(t + 1, NB) * P;
            fa1[d] = FA1[e0]; fa2[d] = FA2[e0]; fs[d] = FSp[e0];
            gA[d] = GA[e1]; gB[d] = GB[e1]; gC[d] = GC[e1];
        }
    };
#pragma unroll
    for (int d = 0; d < SH_ME_D; d++) rows_of((BAND ? T0 : 0) + d, d);
    float Xs[4][SH_ME_K], Xi[4][SH_ME_K], Xd[SH_ME_K - 1], sub[4], ins[4];
    float del = -SH_MAP_BIG;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        sub[c] = -SH_MAP_BIG;
        ins[c] = -SH_MAP_BIG;
#pragma unroll
        for (int m = 0; m < SH_ME_K; m++) { Xs[c][m] = -SH_MAP_BIG; Xi[c][m] = -SH_MAP_BIG; }
    }
#pragma unroll
    for (int m = 0; m < SH_ME_K - 1; m++) Xd[m] = -SH_MAP_BIG;
    __syncthreads();
    const int nchunk = BAND ? (max(T1 - T0, 0) + SH_ME_CH - 1) / SH_ME_CH : (NB + SH_ME_CH - 1) / SH_ME_CH;
    for (int c0 = 0; c0 < nchunk; c0++) {
        const float *const tc = sh_me_cols + (long long)((c0 & 1) * SH_ME_CH) * NRP;
        for (int u0 = 0; u0 < SH_ME_CH; u0 += SH_ME_D) {
#pragma unroll
            for (int d = 0; d < SH_ME_D; d++) {
                const int u = u0 + d, t = (BAND ? T0 : 0) + c0 * SH_ME_CH + u;
                if (t >= (BAND ? T1 : NB)) break;            /* (uniform) */
                const float *const col = tc + (long long)u * NRP;
                const float lps = col[STAY];
                const float ls = VIT ? fmaxf(-local_pen, lps) : sh_lse(-local_pen, lps);
                const float leA = col[sA], leB = col[sB], leC = col[sC];
                sh_me_edit<VIT, SH_ME_K - 1>(Xd, del, cd, zw, 0, A, Md, Jd, Bs, fa2[d], fa1[d], fs[d], col, lps, ls, leB, leC, gB[d], gC[d], stay_pen,
                                             skip_pen, local_pen);
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    sh_me_edit<VIT, SH_ME_K>(Xs[c], sub[c], cs, cw, c, A, Ms, Js, Bs, fa2[d], fa1[d], fs[d], col, lps, ls, leB, leC, gB[d], gC[d],
                                             stay_pen, skip_pen, local_pen);
                    sh_me_edit<VIT, SH_ME_K>(Xi[c], ins[c], ci, cw, c, A, Mi, Ji, Bi, fa2[d], fa1[d], fs[d], col, lps, ls, leA, leB, gA[d], gB[d],
                                             stay_pen, skip_pen, local_pen);
                }
                rows_of(t + SH_ME_D, d);
            }
        }
        stage((c0 + 1) & 1);                                 /* chunk c0 + 1; that buffer was read last in chunk c0 - 1, a barrier ago */
        fetch(c0 + 2);
        __syncthreads();
    }
    if (!mine) return;
    /* no suffix: k_map's end rule on the edit's last column and END's chain */
    float fN;
    if constexpr (BAND) {
        int l, h;
        sh_me_band(blo, NB, NB, l, h);
        fN = cell(F, NB, max(A - 1, 0), l, h);
    } else fN = FA1[(long long)NB * P];
    auto end = [&](float x, float y) { return VIT ? fmaxf(x, y) : sh_lse(x, y); };
    float *const out = a.res + r.res;
    if (Bi == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) ins[c] = end(sh_me_last<SH_ME_K>(Xi[c], Mi, fN), ins[c]);
    }
    *(float4 *)(out + 4 * (long long)L + 4 * (long long)i) = make_float4(ins[0], ins[1], ins[2], ins[3]);
    if (i < L) {
        if (Bs == 0) {
#pragma unroll
            for (int c = 0; c < 4; c++) sub[c] = end(sh_me_last<SH_ME_K>(Xs[c], Ms, fN), sub[c]);
            del = end(sh_me_last<SH_ME_K - 1>(Xd, Md, fN), del);
        }
        *(float4 *)(out + 4 * (long long)i) = make_float4(sub[0], sub[1], sub[2], sub[3]);
        out[8 * (long long)L + 4 + i] = del;
    }
}

#endif /* SH_MAP_EDITS_H */
