/* sh_map_pack.h -- one read mapped to several candidate sequences at once: the unbanded recursion of k_map (sh_map.h,
 * decode.c:1420-1700), scores only, over a PACK of candidates of the same read in one workgroup.
 *
 * Layout: the candidates of a pack are laid end to end, candidate k as the segment [START, s_0 ... s_{L-1}, END] of L_k + 2
 * cells from cell first[k] on; first[ncand] is the pack's cell count.  Two ping-pong rows of ncell floats, one word per cell
 * (its state code, and in the top bits its KIND: START, position 0, position 1, position >= 2, END) and the ncand + 1 words
 * of first[] live in LDS and are loaded once.  Every predecessor of a state cell g is g, g - 1 or g - 2, and its kind says
 * which of them exist (position 0 reads its START at g - 1; position 1 has one left neighbour): nothing reaches across a
 * segment boundary.
 *
 * Work split: one workgroup of SH_MAP_NTH threads per pack, cell g on thread g % SH_MAP_NTH, one barrier per block for the
 * whole pack; the stay entry is fetched once per block.  START, END and the final score are per candidate and belong to thread
 * k % SH_MAP_NTH.  A state cell goes through sh_map_cell, the function k_map's unbanded form goes through, so a candidate's
 * score is the bits k_map gives for it alone, Viterbi and forward.  LDS is the only home (no pointer chooses between LDS and
 * global memory: no flat instruction); a candidate too long for it takes k_map.  No traceback: a path comes from k_map on the
 * one candidate that needs it.
 */
#ifndef SH_MAP_PACK_H
#define SH_MAP_PACK_H

#include "sh_map.h"

enum { SH_MPK_START = 0, SH_MPK_POS0 = 1, SH_MPK_POS1 = 2, SH_MPK_POS2 = 3, SH_MPK_END = 4 };
#define SH_MPK_KIND_SHIFT 28      /* a cell word: kind << 28 | state code (codes stay below 2^28: map_pack_states_ok) */
#define SH_MPK_CODE_MASK 0x0fffffff

struct ShMapPack {
    long long post;     /* as ShMapRead: dense, float offset of the read's row 0; tiled, the read's first column block */
    long long cell;     /* first cell word of the pack in cells[] */
    long long first;    /* first of the pack's ncand + 1 words in firsts[] */
    long long out;      /* where the pack's first candidate's score goes in score[] */
    int nblock, ncell, ncand;
    int lane;           /* tiled: the read's lane in its tile */
};

/* a: post / E / sums / pstride / nr / nchunk / min_prob / the penalties / score as k_map takes them (rd, seq, band, tb, scr and
 * final_state are not used) */
template <bool VIT, bool TILED>
__global__ __launch_bounds__(SH_MAP_NTH) void k_map_pack(ShMapArgs a, const ShMapPack *__restrict__ packs, const int *__restrict__ cells,
                                                         const int *__restrict__ firsts) {
    extern __shared__ float sh_map_lds[];
    const ShMapPack pk = packs[blockIdx.x];
    const int tid = threadIdx.x, NC = pk.ncell, NK = pk.ncand, NB = pk.nblock, STAY = a.nr - 1;
    const float stay_pen = a.stay_pen, skip_pen = a.skip_pen, local_pen = a.local_pen;
    float *const buf0 = sh_map_lds;
    float *const buf1 = buf0 + NC;
    int *const word = (int *)(sh_map_lds + 2 * NC);
    int *const first = word + NC;
    for (int g = tid; g < NC; g += SH_MAP_NTH) {
        const int w = cells[pk.cell + g];
        word[g] = w;
        buf0[g] = (w >> SH_MPK_KIND_SHIFT) == SH_MPK_START ? 0.0f : -SH_MAP_BIG;
        buf1[g] = -SH_MAP_BIG;
    }
    for (int k = tid; k <= NK; k += SH_MAP_NTH) first[k] = firsts[pk.first + k];
    ShMapRead r{};
    r.post = pk.post; r.lane = pk.lane;
    __syncthreads();
    ShMapPost<TILED> lp;
    for (int blk = 0; blk < NB; blk++) {
        const float *p = (blk & 1) ? buf1 : buf0;
        float *c = (blk & 1) ? buf0 : buf1;
        lp.block(a, r, blk);
        const float lps = lp(STAY);
        for (int g = tid; g < NC; g += SH_MAP_NTH) {
            const int w = word[g], kind = w >> SH_MPK_KIND_SHIFT;
            if (kind == SH_MPK_START || kind == SH_MPK_END) continue;
            const float le = lp(w & SH_MPK_CODE_MASK);
            int code = 0;
            c[g] = sh_map_cell<VIT>(p, g, g - 1, kind - SH_MPK_POS0, le, lps, stay_pen, skip_pen, code);
        }
        if (tid < NK) {
            const float ls = VIT ? fmaxf(-local_pen, lps) : sh_lse(-local_pen, lps);
            for (int k = tid; k < NK; k += SH_MAP_NTH) {
                const int s = first[k], en = first[k + 1] - 1;       /* START, END; the last state is en - 1 */
                c[s] = p[s] + ls;
                float e = p[en] + ls;
                const float ex = p[en - 1] - local_pen;
                if (VIT) { if (ex > e) e = ex; }
                else e = sh_lse(e, ex);
                c[en] = e;
            }
        }
        __syncthreads();
    }
    const float *f = (NB & 1) ? buf1 : buf0;
    for (int k = tid; k < NK; k += SH_MAP_NTH) {
        const int en = first[k + 1] - 1;
        const float x = f[en - 1], y = f[en];
        a.score[pk.out + k] = VIT ? fmaxf(x, y) : sh_lse(x, y);
    }
}

#endif /* SH_MAP_PACK_H */
