/* sh_crf_edits.h -- part of sh_kernels.h (included from there, behind sh_map_crf_pack.h): EVERY single-base edit of a sequence scored
 * against a read of a flip-flop (CRF) model in one pass -- 3 L substitutions (and the L that change nothing), L deletions, 4 (L + 1)
 * insertions: what a polisher or a variant caller asks of a window.  Scores only, unbanded.
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
 * below -SH_MAP_BIG / 2: no admissible path (the host answers NAN).  All stores are plain vector stores. */
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

struct ShCrfEditsArgs {
    const ShCrfEditsRead *rd;
    const float *trans;         /* d_E, or the uploaded matrices */
    const int *seq;
    float *rows;
    float *res;
    float *base;                /* [read] */
};

template <bool VIT> __device__ __forceinline__ float sh_ce_mx(float a, float b) { return VIT ? (b > a ? b : a) : sh_lse(a, b); }
template <bool VIT> __device__ __forceinline__ float sh_ce_end(float x, float y) { return VIT ? (x >= y ? x : y) : sh_lse(x, y); }

template <class LOADER>
__device__ __forceinline__ auto sh_ce_view(const float *tr, const ShCrfEditsRead &r) {
    ShMapCrfRead m{};
    m.trans = r.trans; m.lane = r.lane; m.nblock = r.nblock;
    return ShMapCrfView<LOADER>::make(tr, m);
}

template <bool VIT, class LOADER, bool BACK>
__global__ __launch_bounds__(SH_MAP_NTH) void k_crf_edits_rows(ShCrfEditsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_ce_lds[];
    const ShCrfEditsRead r = a.rd[blockIdx.x];
    const int tid = threadIdx.x, L = r.seqlen, NB = r.nblock, RW = L + 2, SPARE = L + 1;
    const long long P = r.pitch, M = (long long)(NB + 1) * P;
    float *const trb = sh_ce_lds;                            /* [2][32] */
    float *const buf0 = sh_ce_lds + SH_MAPC_HEAD;
    float *const buf1 = buf0 + 2 * RW;
    int *const sq = (int *)(sh_ce_lds + SH_MAPC_HEAD + 4 * RW);
    for (int i = tid; i < L; i += SH_MAP_NTH) sq[i] = a.seq[r.seq + i];
    float *const gB = a.rows + r.rows + (BACK ? 2 * M : 0), *const gS = gB + M;      /* (BACK: gS is not used) */
    const int nch = (L + SH_MAP_NTH) / SH_MAP_NTH;           /* chunks of the block loop: cells 0 .. L */
    {
        float *const g0 = gB + (BACK ? (long long)NB * P : 0);
        for (int p = tid; p <= L; p += SH_MAP_NTH) {         /* the first row: entry 0, or entry NB */
            const float b = BACK ? (p == L ? 0.0f : -SH_MAP_BIG) : (p == 1 ? 0.0f : -SH_MAP_BIG);
            const float s = BACK ? (p == L ? 0.0f : -SH_MAP_BIG) : (p == 0 ? 0.0f : -SH_MAP_BIG);
            buf0[p] = b;
            buf0[RW + p] = s;
            g0[p] = b;
            if (!BACK) g0[M + p] = s;
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
            for (int ch = 0; ch < nch; ch++) {
                const int p = ch * SH_MAP_NTH + tid;
                const bool valid = p <= L;
                const int b = sq[min(max(p - 1, 0), L - 1)];            /* seq[p - 1] */
                float vb, vs;
                if (!BACK) {                                 /* k_map_crf's unbanded cell */
                    const int p0 = min(p, L), p1 = min(max(p - 1, 0), L);
                    const int bp = sq[min(max(p - 2, 0), L - 1)];
                    const bool in0 = p <= L, in1 = p >= 1 && p - 1 <= L;
                    const float lB0 = pB[p0], lS0 = pS[p0], lB1 = pB[p1], lS1 = pS[p1];
                    const float B0 = in0 ? lB0 : -SH_MAP_BIG, S0 = in0 ? lS0 : -SH_MAP_BIG;
                    const float B1 = in1 ? lB1 : -SH_MAP_BIG, S1 = in1 ? lS1 : -SH_MAP_BIG;
                    bool kb, ks;
                    sh_map_crf_cell<VIT>(tr, tSS, b, bp, p, B0, S0, B1, S1, vb, vs, kb, ks);
                } else {
                    const int nx = sq[min(p, L - 1)];        /* seq[p]: the next base, where p < L */
                    const float nB = pB[min(p + 1, L)], nS = pS[min(p, L)];
                    const float mvB = tr[5 * nx + b] + nB, stB = tr[20 + b] + nS;
                    const float mvS = tr[5 * nx + 4] + nB, stS = tSS + nS;
                    vb = p < L ? sh_ce_mx<VIT>(mvB, stB) : stB;
                    vs = p < L ? sh_ce_mx<VIT>(mvS, stS) : stS;
                    if (p < 1) vb = -SH_MAP_BIG;             /* there is no B[0] */
                }
                const int at = valid ? p : SPARE;
                cB[at] = vb;
                cS[at] = vs;
                gB[row + at] = vb;
                if (!BACK) gS[row + at] = vs;
            }
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

template <bool VIT, class LOADER>
__global__ __launch_bounds__(SH_MAP_NTH) void k_crf_edits(ShCrfEditsArgs a) {
    __shared__ float trs[2][SH_CE_CH * 32];
    const ShCrfEditsRead r = a.rd[blockIdx.x];
    const int L = r.seqlen, NB = r.nblock, tid = threadIdx.x;
    const int i0 = blockIdx.y * SH_MAP_NTH;
    if (i0 > L) return;                                      /* (uniform) */
    const bool mine = i0 + tid <= L;
    const int i = min(i0 + tid, L);
    const long long P = r.pitch, M = (long long)(NB + 1) * P;
    const float *const FB = a.rows + r.rows + i, *const FS = FB + M;
    const float *const G1 = a.rows + r.rows + 2 * M + min(i + 1, L), *const G2 = a.rows + r.rows + 2 * M + min(i + 2, L);
    const int *const sq = a.seq + r.seq;
    const bool hp = i >= 1;                                  /* a base precedes position i */
    const int pb = sq[max(i - 1, 0)], n0 = sq[min(i, L - 1)], n1 = sq[min(i + 1, L - 1)];
    const auto v = sh_ce_view<LOADER>(a.trans, r);
    const int slot = v.slot(tid & 31), srow = tid >> 5;
    constexpr int NQ = SH_CE_CH * 32 / SH_MAP_NTH;
    float q[NQ];
    auto fetch = [&](int c) {
#pragma unroll
        for (int m = 0; m < NQ; m++) q[m] = v.col(c * SH_CE_CH + srow + m * (SH_MAP_NTH / 32))[slot];
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
        const long long e0 = (long long)min(t, NB) * P, e1 = (long long)min(t + 1, NB) * P;
        fb[d] = FB[e0]; fs[d] = FS[e0]; g1[d] = G1[e1]; g2[d] = G2[e1];
    };
    const float g10 = G1[0], g20 = G2[0];
#pragma unroll
    for (int d = 0; d < SH_CE_D; d++) rows_of(d, d);
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
    const int nchunk = (NB + SH_CE_CH - 1) / SH_CE_CH;
    for (int c0 = 0; c0 < nchunk; c0++) {
        const float *const tc = trs[c0 & 1];
        for (int u0 = 0; u0 < SH_CE_CH; u0 += SH_CE_D) {
#pragma unroll
            for (int d = 0; d < SH_CE_D; d++) {
                const int u = u0 + d, t = c0 * SH_CE_CH + u;
                if (t >= NB) break;                          /* (uniform) */
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
            const long long eN = (long long)NB * P;
            del = sh_ce_end<VIT>(FB[eN], FS[eN]);
        }
        *(float4 *)(out + 4 * (long long)i) = make_float4(sub[0], sub[1], sub[2], sub[3]);
        out[8 * (long long)L + 4 + i] = del;
    }
}

#endif /* SH_CRF_EDITS_H */
