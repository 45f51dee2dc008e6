/* sh_crf_edits.h -- part of sh_kernels.h (included from there, behind sh_map_crf_pack.h): EVERY single-base edit of a sequence scored
 * against a read of a flip-flop (CRF) model in one pass -- 3 L substitutions (and the L that change nothing), L deletions, 4 (L + 1)
 * insertions: what a polisher or a variant caller asks of a window.  Scores only; unbanded, or (the BAND instantiations, at the end of
 * this comment) inside a band of k_map_crf's kind.
 *
 * The lattice is k_map_crf's (sh_map_crf.h states it): after entry t a path is in B[p] (entry t was base seq[p - 1]) or S[p] (a stay),
 * p bases emitted.  Every admissible path is in B[p] exactly once, at the entry that emits base p, so a path score splits there:
 *     F_B[t][p], F_S[t][p]   the best (forward: the sum over) beginnings that are in the cell after entry t: k_map_crf's rows, kept;
 *     G_B[t][p], G_S[t][p]   the best (sum over) continuations from the cell at entry t to the end, B[L] or S[L] at entry NB:
 *         G_B[t][p] = mx(tr_t[5 seq[p] + seq[p - 1]] + G_B[t + 1][p + 1],   tr_t[20 + seq[p - 1]] + G_S[t + 1][p])      (1 <= p)
 *         G_S[t][p] = mx(tr_t[5 seq[p] + 4]          + G_B[t + 1][p + 1],   tr_t[24]              + G_S[t + 1][p])
 *     the move to the next base first (p == L has none), then the stay; G_B[NB][L] = G_S[NB][L] = 0, everything else -SH_MAP_BIG.
 * mx(a, b): b if b > a else a (Viterbi), sh_lse(a, b) (forward).  An edit -- the prefix seq[:i], perhaps a new base c, the suffix seq[j:] --
 * walks the prefix's F columns (F_B[.][i], F_S[.][i]; there is no B[0]), runs the new base's own two cells X_B, X_S down the entries,
 * enters the suffix's first base n = seq[j] (Y[t]: that entry is t) and closes with G_B[t][j + 1]; without a suffix the end rule of
 * k_map_crf closes on the last cells themselves.  "Enter x after y from (PB, PS) at block t": mx(tr_t[5 x + y] + PB, tr_t[5 x + 4] + PS),
 * the stay term alone where there is no y.  include/scrappie_hip.h states the whole definition; tests/test_crf_edits_cpu.py restates it.
 * The build has -ffp-contract=off; the Viterbi form holds additions and compares only.
 *
 * k_crf_edits_rows<VIT, LOADER, BACK>: k_map_crf's unbanded LDS form -- one workgroup of SH_MAP_NTH threads per read, cell p on thread
 * p % SH_MAP_NTH, two ping-pong buffers of a B and an S row of L + 2 floats (cells 0 .. L and the slot that takes the stores of threads
 * without a cell), one barrier per block, columns of transitions SH_MAPC_D blocks ahead through two 32-float LDS columns -- that also
 * stores every completed row to device memory as [entry][cell] floats, `pitch` apart (cells 0 .. L, the spare slot at L + 1 < pitch).
 * !BACK: blocks ascending through sh_map_crf_cell<VIT>, so the rows and `base` are k_map_crf's bits by construction; F_B and F_S are kept.
 * BACK: blocks descending (the loaders' col() clamps any index, so the ring runs down as it runs up), the recursion above; cell L + 1 is a
 * select, not a cell; G_B alone is kept.  Every LDS and vector-memory operation of the block loop is unconditional.  LDS is the only home
 * of the rows: L is at most what k_map_crf's LDS home holds.
 *
 * k_crf_edits<VIT, LOADER>: one thread per position i = 0 .. L, consecutive lanes on consecutive i, SH_MAP_NTH positions per workgroup
 * (grid: read x chunk of positions).  The thread walks the blocks serially: per block it loads F_B[t][i], F_S[t][i], G_B[t + 1][i + 1]
 * and G_B[t + 1][i + 2] (coalesced; columns clamp to L where the edit closes by the end rule and the value is dropped), SH_CE_D blocks
 * ahead, and keeps in registers the four X columns -- sub[i][c] and ins[i][c] share them -- and its nine running scores.  The 25
 * transitions of a block come from LDS, SH_CE_CH blocks staged per barrier, the next chunk already in registers.
 * Results per read at res: sub [L][4], ins [L + 1][4], del [L] (in this order: the float4 stores stay 16-byte aligned); a score
 * below -SH_MAP_BIG / 2: no admissible path (the host answers NAN).  All stores are plain vector stores.
 *
 * BAND = true (ShCrfEditsBandRead: low and high of nblock + 1 int32 each behind the codes; include/scrappie_hip.h states the definition): F and G
 * hold -SH_MAP_BIG outside the band of their entry, the new base's cells X carry none.  The rows kernel has ONE block loop, k_map_crf's -- per
 * entry the cells from the 64-cell group of low on, the previous row read under the previous entry's band, nothing ever cleared; without a band
 * the bounds are the constants 0 and L + 1 and BAND decides the bounds, the first chunk's base and the row index of the global store alone -- and
 * in a band stores an entry's band alone: cell p of entry t at float p - low[t] of its row, the row's last slot (pitch - 1, never a cell: pitch > the widest entry)
 * for the threads without one.  The combining kernel indexes the rows the same way (the index clamped into the row, -SH_MAP_BIG selected outside
 * the band) and walks only the blocks at which one of its workgroup's positions can be alive.  With the full band both run the unbanded
 * arithmetic operand for operand: the same bits.  The combining kernel's BAND differences are a few `if constexpr` lines. */
#ifndef SH_CRF_EDITS_H
#define SH_CRF_EDITS_H

#include "sh_map_crf.h"     /* SH_MAPC_D, SH_MAPC_HEAD, ShMapCrfView, sh_map_crf_cell */

#define SH_CE_CH 32               /* blocks of transitions staged in LDS per barrier of k_crf_edits */
#define SH_CE_D 4                 /* blocks of row values in flight per thread of k_crf_edits */

struct ShCrfEditsRead {
    long long trans;    /* tiled: the first column block of the read's tile; reference layout: float offset of the read's matrix */
    long long seq;      /* offset of the read's base codes */
    long long rows;     /* float offset of F_B in rows[]; F_S (nblock + 1) * pitch floats behind it, G_B as many behind F_S */
    long long res;      /* float offset of the read's results in res[] (a multiple of 4) */
    int nblock, seqlen;
    int lane;           /* tiled: the read's lane in its tile (0..15); reference layout: the matrix's column stride */
    int pitch;          /* floats from one entry's row to the next (>= seqlen + 2) */
};

template <class Rec> struct ShCrfEditsArgsT {
    const Rec *rd;
    const float *trans;         /* d_E, or the uploaded matrices */
    const int *seq;             /* codes, and behind them the bands */
    float *rows;
    float *res;
    float *base;                /* [read] */
};
using ShCrfEditsArgs = ShCrfEditsArgsT<ShCrfEditsRead>;

/* A read in a band: the cells [low[t], high[t]) of entry t, as k_map_crf takes them (nblock + 1 int32 each, in seq[] behind the codes).  An entry's
 * row holds its band's cells alone, cell p at float p - low[t], and the slot at pitch - 1 takes the stores of threads without a cell: pitch is
 * the widest entry's cells and that slot rounded up to 16 (scrappie_hip_crf_edits_band_pitch). */
struct ShCrfEditsBandRead : ShCrfEditsRead {
    long long band;     /* offset in seq[] of low; high the next nblock + 1 */
};
using ShCrfEditsBandArgs = ShCrfEditsArgsT<ShCrfEditsBandRead>;

template <bool VIT> __device__ __forceinline__ float sh_ce_mx(float a, float b) { return VIT ? (b > a ? b : a) : sh_lse(a, b); }
template <bool VIT> __device__ __forceinline__ float sh_ce_end(float x, float y) { return VIT ? (x >= y ? x : y) : sh_lse(x, y); }

template <class LOADER>
__device__ __forceinline__ auto sh_ce_view(const float *tr, const ShCrfEditsRead &r) {
    ShMapCrfRead m{};
    m.trans = r.trans; m.lane = r.lane; m.nblock = r.nblock;
    return ShMapCrfView<LOADER>::make(tr, m);
}

template <bool BAND> using ShCrfEditsArgsOf = std::conditional_t<BAND, ShCrfEditsBandArgs, ShCrfEditsArgs>;

template <bool VIT, class LOADER, bool BACK, bool BAND = false>
__global__ __launch_bounds__(SH_MAP_NTH) void k_crf_edits_rows(ShCrfEditsArgsOf<BAND> a) {
    extern __shared__ __attribute__((aligned(16))) float sh_ce_lds[];
    const auto r = a.rd[blockIdx.x];
    const int tid = threadIdx.x, L = r.seqlen, NB = r.nblock, RW = L + 2, SPARE = L + 1;
    const long long P = r.pitch, M = (long long)(NB + 1) * P;
    float *const trb = sh_ce_lds;                            /* [2][32] */
    float *const buf0 = sh_ce_lds + SH_MAPC_HEAD;
    float *const buf1 = buf0 + 2 * RW;
    int *const sq = (int *)(sh_ce_lds + SH_MAPC_HEAD + 4 * RW);
    for (int i = tid; i < L; i += SH_MAP_NTH) sq[i] = a.seq[r.seq + i];
    float *const gB = a.rows + r.rows + (BACK ? 2 * M : 0), *const gS = gB + M;      /* (BACK: gS is not used) */
    /* BAND: the band of the entry a step reads (lo_p, hi_p) and of the one it completes (lo_c, hi_c), as k_map_crf keeps them */
    const int *blo = nullptr, *bhi = nullptr;
    int lo_p = 0, hi_p = L + 1, lo_c = 0, hi_c = L + 1;
    auto entry = [&](int k) { return min(max(BACK ? NB - 1 - k : k + 1, 0), NB); };      /* the entry that step k completes */
    if constexpr (BAND) {
        blo = a.seq + r.band; bhi = blo + (NB + 1);
        lo_p = blo[BACK ? NB : 0]; hi_p = bhi[BACK ? NB : 0];
        lo_c = blo[entry(0)]; hi_c = bhi[entry(0)];
    }
    {
        float *const g0 = gB + (BACK ? (long long)NB * P : 0);
        for (int p = (BAND ? lo_p : 0) + tid; p < (BAND ? hi_p : L + 1); p += SH_MAP_NTH) {      /* the first row: entry 0, or entry NB */
            const float b = BACK ? (p == L ? 0.0f : -SH_MAP_BIG) : (p == 1 ? 0.0f : -SH_MAP_BIG);
            const float s = BACK ? (p == L ? 0.0f : -SH_MAP_BIG) : (p == 0 ? 0.0f : -SH_MAP_BIG);
            buf0[p] = b;
            buf0[RW + p] = s;
            g0[BAND ? p - lo_p : p] = b;
            if (!BACK) g0[M + (BAND ? p - lo_p : p)] = s;
        }
    }
    const auto v = sh_ce_view<LOADER>(a.trans, r);
    const int slot = v.slot(tid & 31);
    auto blk = [&](int k) { return BACK ? NB - 1 - k : k; };    /* the block of step k (col() clamps it) */
    float q[SH_MAPC_D];                                      /* q[d]: the column of step k0 + d + 1 */
    if (tid < 32) trb[tid] = v.col(blk(0))[slot];
#pragma unroll
    for (int d = 0; d < SH_MAPC_D; d++) q[d] = v.col(blk(d + 1))[slot];
    __syncthreads();
    for (int k0 = 0; k0 < NB; k0 += SH_MAPC_D) {
#pragma unroll
        for (int d = 0; d < SH_MAPC_D; d++) {
            const int k = k0 + d;
            if (k >= NB) break;                              /* (uniform) */
            const long long row = (long long)(BACK ? NB - 1 - k : k + 1) * P;      /* the entry this step completes */
            const float *const pB = (k & 1) ? buf1 : buf0, *const pS = pB + RW;
            float *const cB = (k & 1) ? buf0 : buf1, *const cS = cB + RW;
            const float *const tr = trb + (k & 1) * 32;
            const float tSS = tr[24];
            /* k_map_crf's loop: the band's cells alone, from the 64-cell group of lo_c on; without a band the bounds are 0 and L + 1, constants: cells 0 .. L */
            int lo_n = 0, hi_n = L + 1;
            if constexpr (BAND) { const int en = entry(k + 1); lo_n = blo[en]; hi_n = bhi[en]; }      /* asked for before the barrier */
            const int base = lo_c & ~63;
            const int nchb = (hi_c - base + SH_MAP_NTH - 1) / SH_MAP_NTH;
            for (int ch = 0; ch < nchb; ch++) {
                const int p = base + ch * SH_MAP_NTH + tid;
                const bool valid = p >= lo_c && p < hi_c;
                const int b = sq[min(max(p - 1, 0), L - 1)];            /* seq[p - 1] */
                /* what is read is masked by the band of the entry read: forward as k_map_crf does, without a band too; the recursion back needs no mask then */
                constexpr bool FREE = !BAND && BACK;
                const bool in0 = FREE || (p >= lo_p && p < hi_p);       /* cell p of the entry read */
                float vb, vs;
                if (!BACK) {                                 /* k_map_crf's cell */
                    const int p0 = min(p, L), p1 = min(max(p - 1, 0), L);
                    const int bp = sq[min(max(p - 2, 0), L - 1)];
                    const bool in1 = p - 1 >= lo_p && p - 1 <= hi_p - 1;    /* cell p - 1 (in these words the block loop without a band compiles to the code it was: profiles/edits_band_layer_refactor.txt, section 2) */
                    const float lB0 = pB[p0], lS0 = pS[p0], lB1 = pB[p1], lS1 = pS[p1];
                    const float B0 = in0 ? lB0 : -SH_MAP_BIG, S0 = in0 ? lS0 : -SH_MAP_BIG;
                    const float B1 = in1 ? lB1 : -SH_MAP_BIG, S1 = in1 ? lS1 : -SH_MAP_BIG;
                    bool kb, ks;
                    sh_map_crf_cell<VIT>(tr, tSS, b, bp, p, B0, S0, B1, S1, vb, vs, kb, ks);
                } else {
                    const int nx = sq[min(p, L - 1)];        /* seq[p]: the next base, where p < L */
                    const bool inx = FREE || (p + 1 >= lo_p && p + 1 < hi_p);      /* cell p + 1 of the entry read (never L + 1: hi_p <= L + 1) */
                    const float lB = pB[min(p + 1, L)], lS = pS[min(p, L)];
                    const float nB = inx ? lB : -SH_MAP_BIG, nS = in0 ? lS : -SH_MAP_BIG;
                    const float mvB = tr[5 * nx + b] + nB, stB = tr[20 + b] + nS;
                    const float mvS = tr[5 * nx + 4] + nB, stS = tSS + nS;
                    vb = p < L ? sh_ce_mx<VIT>(mvB, stB) : stB;
                    vs = p < L ? sh_ce_mx<VIT>(mvS, stS) : stS;
                    if (p < 1) vb = -SH_MAP_BIG;             /* there is no B[0] */
                }
                const int at = valid ? p : SPARE;
                const long long gat = !BAND ? (long long)at : valid ? (long long)(p - lo_c) : P - 1;      /* BAND: the row holds the band's cells; its last slot is no cell's */
                cB[at] = vb;
                cS[at] = vs;
                gB[row + gat] = vb;
                if (!BACK) gS[row + gat] = vs;
            }
            if constexpr (BAND) { lo_p = lo_c; hi_p = hi_c; lo_c = lo_n; hi_c = hi_n; }
            if (tid < 32) trb[((k + 1) & 1) * 32 + tid] = q[d];     /* step k + 1's column; read last in step k - 1, a barrier ago */
            q[d] = v.col(blk(k + 1 + SH_MAPC_D))[slot];
            __syncthreads();
        }
    }
    if (!BACK && tid == 0) {
        const float *const f = (NB & 1) ? buf1 : buf0;
        a.base[blockIdx.x] = sh_ce_end<VIT>(f[L], f[RW + L]);
    }
}

template <bool VIT, class LOADER, bool BAND = false>
__global__ __launch_bounds__(SH_MAP_NTH) void k_crf_edits(ShCrfEditsArgsOf<BAND> a) {
    __shared__ float trs[2][SH_CE_CH * 32];
    const auto r = a.rd[blockIdx.x];
    const int L = r.seqlen, NB = r.nblock, tid = threadIdx.x;
    const int i0 = blockIdx.y * SH_MAP_NTH;
    if (i0 > L) return;                                      /* (uniform) */
    const bool mine = i0 + tid <= L;
    const int i = min(i0 + tid, L);
    const long long P = r.pitch, M = (long long)(NB + 1) * P;
    /* BAND: the rows hold the band's cells (cell p of entry t at p - low[t]); FB and G1 = G2 are the matrices' starts, the cell goes into the index.
     * The workgroup walks blocks T0 .. T1 - 1 alone: before entry T0 -- the first whose band reaches its first position's cell, high[T0] > i0 -- every
     * source cell of its positions is outside the band and X, the sums and the maxima hold nothing admissible; from entry T1 on -- the last whose
     * band still holds the cell two behind its last position, low[T1] <= min(i0 + SH_MAP_NTH + 1, L): the furthest G a position joins -- nothing joins.
     * With the end rule (positions L - 1 and L) that cell is L and T1 = NB. */
    const int *blo = nullptr, *bhi = nullptr;
    int T0 = 0, T1 = NB;
    if constexpr (BAND) {
        __shared__ int cnt[2];
        blo = a.seq + r.band; bhi = blo + (NB + 1);
        if (tid < 2) cnt[tid] = 0;
        __syncthreads();
        const int c1 = min(i0 + SH_MAP_NTH + 1, L);
        int below = 0, reach = 0;
        for (int t = tid; t <= NB; t += SH_MAP_NTH) { below += bhi[t] <= i0; reach += blo[t] <= c1; }      /* both edges are non-decreasing: prefixes */
        if (below) atomicAdd(&cnt[0], below);
        if (reach) atomicAdd(&cnt[1], reach);
        __syncthreads();
        T0 = cnt[0]; T1 = cnt[1] - 1;                        /* high[NB] = L + 1 > i0: T0 <= NB; low[0] = 0: T1 >= 0 */
    }
    const float *const FB = a.rows + r.rows + (BAND ? 0 : i), *const FS = FB + M;
    const float *const G1 = a.rows + r.rows + 2 * M + (BAND ? 0 : min(i + 1, L)), *const G2 = a.rows + r.rows + 2 * M + (BAND ? 0 : min(i + 2, L));
    /* BAND: cell c of entry e from the matrix at m; outside the band -SH_MAP_BIG, the index clamped into the row */
    auto cell = [&](const float *m, int e, int c, int lo, int hi) {
        const float x = m[(long long)e * P + min(max(c - lo, 0), (int)P - 1)];
        return c >= lo && c < hi ? x : -SH_MAP_BIG;
    };
    const int *const sq = a.seq + r.seq;
    const bool hp = i >= 1;                                  /* a base precedes position i */
    const int pb = sq[max(i - 1, 0)], n0 = sq[min(i, L - 1)], n1 = sq[min(i + 1, L - 1)];
    const auto v = sh_ce_view<LOADER>(a.trans, r);
    const int slot = v.slot(tid & 31), srow = tid >> 5;
    constexpr int NQ = SH_CE_CH * 32 / SH_MAP_NTH;
    float q[NQ];
    auto fetch = [&](int c) {
#pragma unroll
        for (int m = 0; m < NQ; m++) q[m] = v.col((BAND ? T0 : 0) + c * SH_CE_CH + srow + m * (SH_MAP_NTH / 32))[slot];
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int m = 0; m < NQ; m++) trs[buf][(srow + m * (SH_MAP_NTH / 32)) * 32 + (tid & 31)] = q[m];
    };
    fetch(0);
    stage(0);
    fetch(1);
    /* block t reads the prefix's cells of entry t and the suffix's of entry t + 1 */
    float fb[SH_CE_D], fs[SH_CE_D], g1[SH_CE_D], g2[SH_CE_D];
    auto rows_of = [&](int t, int d) {
        if constexpr (BAND) {
            const int t0 = min(t, NB), t1 = min(t + 1, NB);
            const int l0 = blo[t0], h0 = bhi[t0], l1 = blo[t1], h1 = bhi[t1];
            fb[d] = cell(FB, t0, i, l0, h0); fs[d] = cell(FS, t0, i, l0, h0);
            g1[d] = cell(G1, t1, min(i + 1, L), l1, h1); g2[d] = cell(G2, t1, min(i + 2, L), l1, h1);
        } else {
            const long long e0 = (long long)min(t, NB) * P, e1 = (long long)min(t + 1, NB) * P;
            fb[d] = FB[e0]; fs[d] = FS[e0]; g1[d] = G1[e1]; g2[d] = G2[e1];
        }
    };
    float g10, g20;                                          /* G_B[T0][i + 1], G_B[T0][i + 2] */
    if constexpr (BAND) {
        const int l = blo[min(T0, NB)], h = bhi[min(T0, NB)];
        g10 = cell(G1, min(T0, NB), min(i + 1, L), l, h); g20 = cell(G2, min(T0, NB), min(i + 2, L), l, h);
    } else {
        g10 = G1[0]; g20 = G2[0];
    }
#pragma unroll
    for (int d = 0; d < SH_CE_D; d++) rows_of(T0 + d, d);
    float XB[4], XS[4], sub[4], ins[4];
    float del = (i == 0 ? 0.0f : -SH_MAP_BIG) + g20;         /* entry 0 is the suffix's first base only where nothing precedes it */
#pragma unroll
    for (int c = 0; c < 4; c++) {
        XB[c] = i == 0 ? 0.0f : -SH_MAP_BIG;
        XS[c] = -SH_MAP_BIG;
        sub[c] = -SH_MAP_BIG + g20;
        ins[c] = -SH_MAP_BIG + g10;
    }
    __syncthreads();
    const int nchunk = BAND ? (max(T1 - T0, 0) + SH_CE_CH - 1) / SH_CE_CH : (NB + SH_CE_CH - 1) / SH_CE_CH;
    for (int c0 = 0; c0 < nchunk; c0++) {
        const float *const tc = trs[c0 & 1];
        for (int u0 = 0; u0 < SH_CE_CH; u0 += SH_CE_D) {
#pragma unroll
            for (int d = 0; d < SH_CE_D; d++) {
                const int u = u0 + d, t = (BAND ? T0 : 0) + c0 * SH_CE_CH + u;
                if (t >= (BAND ? T1 : NB)) break;            /* (uniform) */
                const float *const tr = tc + u * 32;
                const float tSS = tr[24], e1 = tr[5 * n1 + 4], e0 = tr[5 * n0 + 4];
                const float dB = tr[5 * n1 + pb] + fb[d], dS = e1 + fs[d];
                const float yd = hp ? sh_ce_mx<VIT>(dB, dS) : dS;
                del = sh_ce_mx<VIT>(del, yd + g2[d]);
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float ys = sh_ce_mx<VIT>(tr[5 * n1 + c] + XB[c], e1 + XS[c]);
                    sub[c] = sh_ce_mx<VIT>(sub[c], ys + g2[d]);
                    const float yi = sh_ce_mx<VIT>(tr[5 * n0 + c] + XB[c], e0 + XS[c]);
                    ins[c] = sh_ce_mx<VIT>(ins[c], yi + g1[d]);
                    const float xB = tr[5 * c + pb] + fb[d], xS = tr[5 * c + 4] + fs[d];
                    const float nb = hp ? sh_ce_mx<VIT>(xB, xS) : xS;
                    const float ns = sh_ce_mx<VIT>(tr[20 + c] + XB[c], tSS + XS[c]);
                    XB[c] = nb;
                    XS[c] = ns;
                }
                rows_of(t + SH_CE_D, d);
            }
        }
        stage((c0 + 1) & 1);                                 /* chunk c0 + 1; that buffer was read last in chunk c0 - 1, a barrier ago */
        fetch(c0 + 2);
        __syncthreads();
    }
    if (!mine) return;
    float *const out = a.res + r.res;
    if (i == L) {                                            /* no suffix: the end rule on the new base's cells */
#pragma unroll
        for (int c = 0; c < 4; c++) ins[c] = sh_ce_end<VIT>(XB[c], XS[c]);
    }
    *(float4 *)(out + 4 * (long long)L + 4 * (long long)i) = make_float4(ins[0], ins[1], ins[2], ins[3]);
    if (i < L) {
        if (i == L - 1) {
#pragma unroll
            for (int c = 0; c < 4; c++) sub[c] = sh_ce_end<VIT>(XB[c], XS[c]);
            if constexpr (BAND) {
                const int l = blo[NB], h = bhi[NB];
                del = sh_ce_end<VIT>(cell(FB, NB, i, l, h), cell(FS, NB, i, l, h));
            } else {
                const long long eN = (long long)NB * P;
                del = sh_ce_end<VIT>(FB[eN], FS[eN]);
            }
        }
        *(float4 *)(out + 4 * (long long)i) = make_float4(sub[0], sub[1], sub[2], sub[3]);
        out[8 * (long long)L + 4 + i] = del;
    }
}

#endif /* SH_CRF_EDITS_H */
