/* sh_crf_find.h -- part of sh_kernels.h (included from there, behind sh_map_crf.h): short sequences (motifs: a barcode, an adapter, a
 * primer) searched INSIDE a read of a flip-flop (CRF) model.  decode_crf's recursion (decode.c:836-893) restricted to the paths
 * that hold the motif: there are entries begin <= end, both bases, such that the non-stay entries in [begin, end] are exactly
 * m[0..L) in order; the entries before begin and behind end are free.  Viterbi only: a path whose call holds the motif twice has
 * several decompositions, so a sum over (path, begin, end) would count it more than once.
 *
 * A read's transitions: 25 floats per block, element to * 5 + from, states A C G T stay (4).  The lattice at one entry:
 *     U[s], s = 0..4       no motif base emitted yet, the entry's state is s: decode_crf's own row
 *     B[p], S[p], p = 1 .. L - 1   p motif bases emitted, the entry is base m[p - 1] (B) or a stay (S): k_map_crf's cells
 *     V[s], s = 0..4       all L bases emitted, the entry's state is s
 * Entry 0: U[s] = 0; B[1] = 0 (begin 0) where L >= 2, V[m[0]] = 0 (begin = end = 0) where L == 1; everything else -SH_MAP_BIG.
 * Block t (entry t -> t + 1), in float32 as tr + prev, every maximum over its candidates in the order written, replaced on
 * strict >:
 *     U'[s'] = max_s tr[5 s' + s] + U[s]                                   s ascending
 *     B'[1]  = max_s tr[5 m0 + s] + U[s]                                   s ascending; begin = t + 1
 *     B'[p]  = max(tr[5 b + m[p - 2]] + B[p - 1], tr[5 b + 4] + S[p - 1])  b = m[p - 1], 2 <= p <= L - 1
 *     S'[p]  = max(tr[20 + b] + B[p], tr[24] + S[p])                       1 <= p <= L - 1
 *     V'[s'] = max_s tr[5 s' + s] + V[s]                                   s ascending, (begin, end) of the winner; then, for
 *              s' == m[L - 1] only, L >= 2: tr[5 s' + m[L - 2]] + B[L - 1], tr[5 s' + 4] + S[L - 1] (end = t + 1);
 *                                   L == 1: tr[5 s' + s] + U[s], s ascending (begin = end = t + 1)
 * End: the first maximum of V[s] at entry NB, s ascending, and that cell's (begin, end); below -SH_MAP_BIG / 2 no occurrence fits
 * (L > NB + 1; the host answers NAN).  call_score: the first maximum of U[s] at entry NB, decode_crf's score bit for bit.  Float
 * addition is monotone, so score <= call_score, with equality in bits where the motif is a run of the call's own bases.  The
 * build has -ffp-contract=off, and the recursion holds additions and compares only.
 *
 * Layout, as k_map_pack: one workgroup of SH_MAP_NTH threads per PACK of motifs of one read.  Cells 0 .. 4 are the read's U cells,
 * once per pack; then every motif's L - 1 interior cells (B[p] and S[p] share cell p) and its five V cells, end to end.  One word
 * per cell: its kind, the state of a U or V cell, the base codes it needs (m[p - 1], m[p - 2]; m[L - 1], m[L - 2] in a V cell) and,
 * in a V cell, the motif's index in the pack.  An interior cell reads itself and its left neighbour, a V cell its motif's five V
 * cells and the cell in front of them: nothing reaches across a segment boundary except to the U cells.
 * Per buffer a row of values (U, B or V) and a row of S; with POS two rows of int32 more: the begin of B and of S, or (begin, end)
 * of a V cell.  Rows hold ncell + 1 entries: the last takes the stores of threads without a cell, which run the U recursion of
 * state 0 on it.  Two ping-pong buffers, one barrier per block for the whole pack; LDS is the only home (no pointer chooses
 * between LDS and global memory, no flat instruction): (SH_MAPC_HEAD + (POS ? 9 : 5) (ncell + 1)) * 4 bytes.
 * Cell g runs on thread g % SH_MAP_NTH.  Transitions as in k_map_crf: thread e & 31 loads element slot(e) of a column SH_MAPC_D
 * blocks ahead, through the loaders' views of sh_crf_post.h, and hands it over through two 32-float LDS columns; the columns clamp,
 * so every vector-memory operation of the block loop is unconditional.  Results per motif (score, begin and end) by plain vector
 * stores from the thread that owns its first V cell, the pack's call_score from the thread of cell 0.  No traceback. */
#ifndef SH_CRF_FIND_H
#define SH_CRF_FIND_H

#include "sh_map_crf.h"     /* SH_MAPC_D, SH_MAPC_HEAD, ShMapCrfView */

enum { SH_CFD_U = 0, SH_CFD_B1 = 1, SH_CFD_INT = 2, SH_CFD_V = 3, SH_CFD_V1 = 4 };      /* V1: a V cell of a motif of one base */
/* a cell word: motif in pack << 16 | kind << 12 | state << 8 | b << 4 | bp */
#define SH_CFD_WORD(motif, kind, s, b, bp) ((int)(((unsigned)(motif) << 16) | ((unsigned)(kind) << 12) | ((unsigned)(s) << 8) | ((unsigned)(b) << 4) | (unsigned)(bp)))

struct ShCrfFindPack {
    long long trans;    /* tiled: the first column block of the read's tile; reference layout: float offset of the read's matrix */
    long long cell;     /* first cell word of the pack in cells[] */
    long long out;      /* where the pack's first motif's results go in score[] / pos[] */
    int nblock, ncell;
    int lane;           /* tiled: the read's lane in its tile (0..15); reference layout: the matrix's column stride */
    int pad;
};

struct ShCrfFindArgs {
    const ShCrfFindPack *packs;
    const float *trans;         /* d_E, or the uploaded matrices */
    const int *cells;
    float *score;               /* [motif] */
    int2 *pos;                  /* [motif] (begin, end); POS only */
    float *call;                /* [pack] */
};

template <bool POS, class LOADER>
__global__ __launch_bounds__(SH_MAP_NTH) void k_crf_find(ShCrfFindArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_cfd_lds[];
    const ShCrfFindPack pk = a.packs[blockIdx.x];
    const int tid = threadIdx.x, NC = pk.ncell, NB = pk.nblock, RW = NC + 1;
    float *const trb = sh_cfd_lds;                           /* [2][32] */
    float *const val = sh_cfd_lds + SH_MAPC_HEAD;            /* [2][2][RW]: buffer, {U / B / V, S} */
    int *const pay = (int *)(val + 4 * RW);                  /* POS: [2][2][RW]: buffer, {begin of B or V, begin of S / end of V} */
    int *const word = (int *)(val + (POS ? 8 : 4) * RW);
    const int nch = (NC + SH_MAP_NTH - 1) / SH_MAP_NTH;      /* chunks of the block loop: cells 0 .. NC - 1 */
    for (int g = tid; g <= NC; g += SH_MAP_NTH) {            /* entry 0, the spare slot's word and values included */
        const int w = g < NC ? a.cells[pk.cell + g] : SH_CFD_WORD(0, SH_CFD_U, 0, 0, 0);
        const int kind = (w >> 12) & 15, s = (w >> 8) & 15, b = (w >> 4) & 15;
        word[g] = w;
        val[g] = (kind == SH_CFD_U || kind == SH_CFD_B1 || (kind == SH_CFD_V1 && s == b)) ? 0.0f : -SH_MAP_BIG;
        val[RW + g] = -SH_MAP_BIG;
        if (POS) { pay[g] = 0; pay[RW + g] = 0; }
    }
    ShMapCrfRead r{};
    r.trans = pk.trans; r.lane = pk.lane; r.nblock = NB;
    const auto v = ShMapCrfView<LOADER>::make(a.trans, r);
    const int slot = v.slot(tid & 31);
    float q[SH_MAPC_D];                                      /* q[d]: the column of block t0 + d + 1 */
    if (tid < 32) trb[tid] = v.col(0)[slot];
#pragma unroll
    for (int d = 0; d < SH_MAPC_D; d++) q[d] = v.col(d + 1)[slot];
    __syncthreads();
    for (int t0 = 0; t0 < NB; t0 += SH_MAPC_D) {
#pragma unroll
        for (int d = 0; d < SH_MAPC_D; d++) {
            const int t = t0 + d;                            /* block t: entry t -> entry t + 1 */
            if (t >= NB) break;                              /* (uniform) */
            const float *const pA = val + (t & 1) * 2 * RW, *const pS = pA + RW;
            float *const cA = val + ((t + 1) & 1) * 2 * RW, *const cS = cA + RW;
            const int *const pPA = pay + (t & 1) * 2 * RW, *const pPS = pPA + RW;
            int *const cPA = pay + ((t + 1) & 1) * 2 * RW, *const cPS = cPA + RW;
            const float *const tr = trb + (t & 1) * 32;
            const float tSS = tr[24];
            for (int ch = 0; ch < nch; ch++) {
                const int g = min(ch * SH_MAP_NTH + tid, NC);      /* threads past the pack: the spare slot */
                const int w = word[g];
                const int kind = (w >> 12) & 15, s = (w >> 8) & 15, b = (w >> 4) & 15, bp = w & 15;
                float va, vs = -SH_MAP_BIG;
                int ba = 0, bs = 0;
                if (kind == SH_CFD_INT) {
                    const float x = tr[5 * b + bp] + pA[g - 1], y = tr[5 * b + 4] + pS[g - 1];
                    const bool k = y > x;
                    va = k ? y : x;
                    if (POS) ba = k ? pPS[g - 1] : pPA[g - 1];
                } else {
                    /* five sources, ascending: the U cells (U, B1) or the motif's own V cells */
                    const int src = (kind == SH_CFD_V || kind == SH_CFD_V1) ? g - s : 0;
                    const int to = kind == SH_CFD_B1 ? b : s;
                    const float *const trow = tr + 5 * to;
                    va = trow[0] + pA[src];
                    int k = 0;
#pragma unroll
                    for (int f = 1; f < 5; f++) {
                        const float c = trow[f] + pA[src + f];
                        if (c > va) { va = c; k = f; }
                    }
                    if (POS) {
                        ba = kind == SH_CFD_B1 ? t + 1 : pPA[src + k];
                        bs = pPS[src + k];                   /* a V cell's end (nothing a U or B1 cell keeps) */
                    }
                    if (kind == SH_CFD_V && s == b) {        /* the last base's emission, from the cell in front of the V cells */
                        const int in = src - 1;
                        const float x = tr[5 * s + bp] + pA[in], y = tr[5 * s + 4] + pS[in];
                        if (x > va) { va = x; if (POS) { ba = pPA[in]; bs = t + 1; } }
                        if (y > va) { va = y; if (POS) { ba = pPS[in]; bs = t + 1; } }
                    }
                    if (kind == SH_CFD_V1 && s == b) {       /* a motif of one base: emitted from any U cell */
#pragma unroll
                        for (int f = 0; f < 5; f++) {
                            const float c = trow[f] + pA[f];
                            if (c > va) { va = c; if (POS) { ba = t + 1; bs = t + 1; } }
                        }
                    }
                }
                if (kind == SH_CFD_B1 || kind == SH_CFD_INT) {
                    const float x = tr[20 + b] + pA[g], y = tSS + pS[g];
                    const bool k = y > x;
                    vs = k ? y : x;
                    if (POS) bs = k ? pPS[g] : pPA[g];
                }
                cA[g] = va;
                cS[g] = vs;
                if (POS) { cPA[g] = ba; cPS[g] = bs; }
            }
            if (tid < 32) trb[((t + 1) & 1) * 32 + tid] = q[d];     /* block t + 1's column; read last in block t - 1, a barrier ago */
            q[d] = v.col(t + 1 + SH_MAPC_D)[slot];
            __syncthreads();
        }
    }
    const float *const fA = val + (NB & 1) * 2 * RW;
    const int *const fPA = pay + (NB & 1) * 2 * RW, *const fPS = fPA + RW;
    for (int g = tid; g < NC; g += SH_MAP_NTH) {
        const int w = word[g];
        const int kind = (w >> 12) & 15, s = (w >> 8) & 15;
        if (s != 0 || kind == SH_CFD_B1 || kind == SH_CFD_INT) continue;
        float best = fA[g];                                  /* the first maximum of the five, ascending */
        int k = 0;
        for (int f = 1; f < 5; f++)
            if (fA[g + f] > best) { best = fA[g + f]; k = f; }
        if (kind == SH_CFD_U) a.call[blockIdx.x] = best;
        else {
            const long long o = pk.out + (long long)((unsigned)w >> 16);
            a.score[o] = best;
            if (POS) a.pos[o] = make_int2(fPA[g + k], fPS[g + k]);
        }
    }
}

#endif /* SH_CRF_FIND_H */
