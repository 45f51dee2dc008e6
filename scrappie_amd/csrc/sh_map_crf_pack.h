/* sh_map_crf_pack.h -- part of sh_kernels.h (included from there, behind sh_map_crf.h): one read of a flip-flop (CRF) model against MANY
 * candidate base sequences -- alleles, references, edits of its own call -- in one pass.  Scores only: k_map_crf's unbanded recursion
 * (its header states it), candidate by candidate, through the same cell function (sh_map_crf_cell), so a candidate's score has the bits
 * k_map_crf gives for it alone, Viterbi and forward.  No traceback, no bands: the path of the winner is a second pass of k_map_crf.
 *
 * Layout, as k_crf_find: one workgroup of SH_MAP_NTH threads per PACK of candidates of one read.  Candidate k of L_k bases is the segment
 * of L_k + 1 cells (p = 0 .. L_k; B[p] and S[p] share cell p) from its first cell on; the candidates lie end to end.  One word per cell:
 * its kind -- p == 0, p == 1 or p >= 2 --, the two base codes it needs (seq[p - 1], seq[p - 2]) and, on a candidate's last cell, a flag
 * and the candidate's index in the pack.  A cell reads itself and its left neighbour only, and its kind says which terms exist (p == 0 has
 * no left neighbour of its own: the select drops what the clamped index read), so nothing reaches across a segment boundary.
 * Rows: two ping-pong buffers, each a B row and an S row of ncell + 1 floats: the last slot takes the stores of threads without a cell,
 * which run a p == 0 cell on it.  Cell g runs on thread g % SH_MAP_NTH; one barrier per block for the whole pack.  LDS is the only home
 * (no pointer chooses between LDS and global memory): (SH_MAPC_HEAD + 5 (ncell + 1)) * 4 bytes within SH_MAP_LDS.
 * Transitions as in k_map_crf: thread e & 31 loads element slot(e) of a column SH_MAPC_D blocks ahead, through the loaders' views of
 * sh_crf_post.h, and hands it over through two 32-float LDS columns; the columns clamp, indices clamp and selects drop values, so every
 * LDS and vector-memory operation of the block loop is unconditional.  score[out + k] by a plain vector store from the thread that owns
 * candidate k's last cell; a score below -SH_MAP_BIG / 2: no admissible path (the host answers NAN). */
#ifndef SH_MAP_CRF_PACK_H
#define SH_MAP_CRF_PACK_H

#include "sh_map_crf.h"     /* SH_MAPC_D, SH_MAPC_HEAD, ShMapCrfView, sh_map_crf_cell */

/* a cell word: candidate in pack << 16 | last cell << 15 | kind (min(p, 2)) << 12 | b << 4 | bp */
#define SH_MCP_WORD(cand, last, kind, b, bp) ((int)(((unsigned)(cand) << 16) | ((unsigned)(last) << 15) | ((unsigned)(kind) << 12) | ((unsigned)(b) << 4) | (unsigned)(bp)))

struct ShMapCrfPack {
    long long trans;    /* tiled: the first column block of the read's tile; reference layout: float offset of the read's matrix */
    long long cell;     /* first cell word of the pack in cells[] */
    long long out;      /* where the pack's first candidate's score goes in score[] */
    int nblock, ncell;
    int lane;           /* tiled: the read's lane in its tile (0..15); reference layout: the matrix's column stride */
    int pad;
};

struct ShMapCrfPackArgs {
    const ShMapCrfPack *packs;
    const float *trans;         /* d_E, or the uploaded matrices */
    const int *cells;
    float *score;               /* [candidate] */
};

template <bool VIT, class LOADER>
__global__ __launch_bounds__(SH_MAP_NTH) void k_map_crf_pack(ShMapCrfPackArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_mcp_lds[];
    const ShMapCrfPack pk = a.packs[blockIdx.x];
    const int tid = threadIdx.x, NC = pk.ncell, NB = pk.nblock, RW = NC + 1;
    float *const trb = sh_mcp_lds;                           /* [2][32] */
    float *const val = sh_mcp_lds + SH_MAPC_HEAD;            /* [2][2][RW]: buffer, {B, S} */
    int *const word = (int *)(val + 4 * RW);
    const int nch = (NC + SH_MAP_NTH - 1) / SH_MAP_NTH;      /* chunks of the block loop: cells 0 .. NC - 1 */
    for (int g = tid; g <= NC; g += SH_MAP_NTH) {            /* entry 0, the spare slot's word and values included */
        const int w = g < NC ? a.cells[pk.cell + g] : SH_MCP_WORD(0, 0, 0, 0, 0);
        const int kind = (w >> 12) & 3;
        word[g] = w;
        val[g] = kind == 1 ? 0.0f : -SH_MAP_BIG;             /* B[1] = 0 */
        val[RW + g] = (kind == 0 && g < NC) ? 0.0f : -SH_MAP_BIG;      /* S[0] = 0 */
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
            const float *const pB = val + (t & 1) * 2 * RW, *const pS = pB + RW;
            float *const cB = val + ((t + 1) & 1) * 2 * RW, *const cS = cB + RW;
            const float *const tr = trb + (t & 1) * 32;
            const float tSS = tr[24];
            for (int ch = 0; ch < nch; ch++) {
                const int g = min(ch * SH_MAP_NTH + tid, NC);      /* threads past the pack: the spare slot */
                const int g1 = max(g - 1, 0);
                const int w = word[g];
                const int kind = (w >> 12) & 3, b = (w >> 4) & 3, bp = w & 3;
                const float B0 = pB[g], S0 = pS[g], lB1 = pB[g1], lS1 = pS[g1];
                const float B1 = kind >= 1 ? lB1 : -SH_MAP_BIG, S1 = kind >= 1 ? lS1 : -SH_MAP_BIG;
                float vb, vs;
                bool kb, ks;
                sh_map_crf_cell<VIT>(tr, tSS, b, bp, kind, B0, S0, B1, S1, vb, vs, kb, ks);
                cB[g] = vb;
                cS[g] = vs;
            }
            if (tid < 32) trb[((t + 1) & 1) * 32 + tid] = q[d];     /* block t + 1's column; read last in block t - 1, a barrier ago */
            q[d] = v.col(t + 1 + SH_MAPC_D)[slot];
            __syncthreads();
        }
    }
    const float *const fB = val + (NB & 1) * 2 * RW, *const fS = fB + RW;
    for (int g = tid; g < NC; g += SH_MAP_NTH) {             /* entry NB: a candidate's cell L */
        const int w = word[g];
        if (!((w >> 15) & 1)) continue;
        const float x = fB[g], y = fS[g];
        a.score[pk.out + (long long)((unsigned)w >> 16)] = VIT ? (x >= y ? x : y) : sh_lse(x, y);
    }
}

#endif /* SH_MAP_CRF_PACK_H */
