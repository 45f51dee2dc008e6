/* sh_squig_pack.h -- one raw signal matched to several candidate squiggles at once: the recursion of k_squig (sh_squig.h,
 * decode.c:1109-1193), scores only, over a PACK of candidates of the same read in one workgroup.
 *
 * Layout: the candidates of a pack are laid end to end, candidate k as the npos_k cells from cell first[k] on; a cell is a
 * position and its back state, which share an emission.  START and END are not cells: they belong to the candidate.  Cell g
 * runs on thread g % SH_SQ_NTH.  LDS is the only home (sh_internal.h counts its words): per cell two ping-pong rows of
 * (position, back) values, the five table entries k_squig stages (loc, scale, logsc and the move and stay penalty of its
 * position state) and two words -- A: position in its candidate, the candidate, and which neighbours exist; B: its END
 * piece --; per candidate its first cell, npos, its pieces, START's two values, move / stay of START, stay of END, and END
 * with its step and skip terms.  No cell reads across a segment boundary: where k_squig reads p[st - 1] or p[st - 2] and that
 * is START, the cell reads its candidate's START; where it reads p[pos + 2] or takes part in END as an origin, word A says
 * whether that neighbour exists (the loads themselves are clamped into the pack and unconditional).
 *
 * The recursion is k_squig's, operation for operation and in its order, the comparisons strict >; the emission is sq_emit;
 * forward is the same with sh_lse / sq_lse0.  With -ffp-contract=off a candidate's Viterbi score is the bits k_squig gives
 * for it alone.
 *
 * START, END and the final score of the pack's k-th candidate belong to thread k % SH_SQ_NTH, its owner.  END of a candidate
 * is per sample the first maximum over its origins 1 .. npos - 1: a SEGMENTED reduction.  Every group of 64 consecutive
 * cells is one wave in one chunk; the wave reduces (value, origin) pairs with shuffles, a lane taking its neighbour d lanes up
 * only where that lane is of the same candidate (ties to the smaller origin), so the first lane of each candidate's stretch in
 * the group -- a PIECE, at most ceil(npos / 64) + 1 per candidate -- ends with the stretch's pair and leaves it in the
 * piece's LDS slot t & 1.  Which piece a cell belongs to and whether it heads it is in word B, from the host
 * (sh_host.c: sh_squig_pack_layout); the kernel computes no piece index.  After the sample's one barrier, at the top of
 * iteration t + 1, the owner folds stay, step, skip and then its candidate's pieces in their order, as thread 0 of k_squig
 * folds its four waves: END trails by one sample, and no second barrier is needed.  The pairs are kept in Viterbi although
 * nothing is traced back, so END's chain of comparisons is k_squig's.  The order of the forward sum is free.
 */
#ifndef SH_SQUIG_PACK_H
#define SH_SQUIG_PACK_H

#include "sh_squig.h"
#include "sh_internal.h"

struct ShSquigPack {
    long long sig;      /* float offset of the read's first sample */
    long long cell;     /* first word of the pack's tables in words[]: 7 ncell + 7 ncand words (sh_internal.h) */
    long long out;      /* where the pack's first candidate's score goes in score[] */
    int nsample, ncell, ncand, npiece;
};

struct ShSquigPackArgs {
    const ShSquigPack *pk;
    const float *sig;
    const int *words;
    float *score;
    float move_back_pen, half_pen;      /* logf(prob_back), logf(0.5f) */
    float local_pen, skip_pen, minscore;
};

template <bool VIT>
__global__ __launch_bounds__(SH_SQ_NTH) void k_squig_pack(ShSquigPackArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_sqp_lds[];
    const ShSquigPack pk = a.pk[blockIdx.x];
    const int tid = threadIdx.x, NC = pk.ncell, NK = pk.ncand, NPC = pk.npiece, NS = pk.nsample;
    /* what the host sent, in its order */
    const float *const loc = sh_sqp_lds, *const scale = loc + NC, *const logsc = scale + NC, *const move = logsc + NC, *const stay = move + NC;
    const int *const wordA = (const int *)(stay + NC), *const wordB = wordA + NC;
    const int *const first = wordB + NC, *const npos = first + NK, *const piece0 = npos + NK, *const npiece = piece0 + NK;
    const float *const move0 = (const float *)(npiece + NK), *const stay0 = move0 + NK, *const stayE = stay0 + NK;
    const int nin = SH_SQP_IN_CELL_WORDS * NC + SH_SQP_IN_CAND_WORDS * NK;
    /* the kernel's own */
    float *const start = sh_sqp_lds + nin;                  /* [2][NK] */
    float *const endv = start + 2 * NK, *const estep = endv + NK, *const eskip = estep + NK;
    float *const rowP = eskip + NK, *const rowB = rowP + 2 * NC;      /* [2][NC] each */
    float *const part_v = rowB + 2 * NC;                    /* [2][NPC] */
    int *const part_o = (int *)(part_v + 2 * NPC);
    {
        const int *const src = a.words + pk.cell;
        int *const dst = (int *)sh_sqp_lds;
        for (int i = tid; i < nin; i += SH_SQ_NTH) dst[i] = src[i];
    }
    for (int g = tid; g < 2 * NC; g += SH_SQ_NTH) { rowP[g] = -SH_MAP_BIG; rowB[g] = -SH_MAP_BIG; }
    for (int k = tid; k < NK; k += SH_SQ_NTH) { start[k] = 0.0f; start[NK + k] = -SH_MAP_BIG; endv[k] = -SH_MAP_BIG; estep[k] = 0.0f; eskip[k] = 0.0f; }
    const float *const sig = a.sig + pk.sig;
    const float local_pen = a.local_pen, skip_pen = a.skip_pen, minscore = a.minscore, back_pen = a.move_back_pen, half_pen = a.half_pen;
    const int nch = (NC + SH_SQ_NTH - 1) / SH_SQ_NTH, ln = tid & 63;
    float x = sig[0];
    __syncthreads();
    for (int t = 0; t <= NS; t++) {
        const float *pP = rowP + (t & 1) * NC, *pB = rowB + (t & 1) * NC, *pS = start + (t & 1) * NK;
        float *cP = rowP + ((t + 1) & 1) * NC, *cB = rowB + ((t + 1) & 1) * NC, *cS = start + ((t + 1) & 1) * NK;
        for (int k = tid; k < NK; k += SH_SQ_NTH) {      /* the owner: END of row t from row t - 1, then row t's step and skip terms */
            const int last = first[k] + npos[k] - 1;
            if (t > 0) {
                const float *pv = part_v + ((t - 1) & 1) * NPC + piece0[k];
                const int *po = part_o + ((t - 1) & 1) * NPC + piece0[k];
                const int np = npiece[k];
                float e = endv[k] + stayE[k];
                if (VIT) {
                    const float e_step = estep[k], e_skip = eskip[k];
                    if (e_step > e) e = e_step;
                    if (e_skip > e) e = e_skip;
                    float bv = pv[0];
                    int bo = po[0];
                    for (int w = 1; w < np; w++) {
                        const float ov = pv[w];
                        const int oo = po[w];
                        if (ov > bv || (ov == bv && oo < bo)) { bv = ov; bo = oo; }
                    }
                    if (bv > e) e = bv;
                } else {
                    e = sh_lse(e, estep[k]);
                    e = sh_lse(e, eskip[k]);
                    float acc = pv[0];
                    for (int w = 1; w < np; w++) acc = sq_lse0(acc, pv[w]);
                    if (acc != -INFINITY) e = sh_lse(e, acc);
                }
                endv[k] = e - local_pen;
            }
            if (t < NS) {
                estep[k] = pP[last] + move[last];
                const bool two = npos[k] >= 2;
                const int lm = two ? last - 1 : last;
                eskip[k] = ((two ? pP[lm] : pS[k]) + (two ? move[lm] : move0[k])) - skip_pen;
                cS[k] = (pS[k] + stay0[k]) - local_pen;
            }
        }
        if (t == NS) break;
        const float xn = sig[t + 1 < NS ? t + 1 : t];      /* the next sample, asked for before the barrier */
        for (int ch = 0; ch < nch; ch++) {
            const int g = ch * SH_SQ_NTH + tid;
            const bool valid = g < NC;
            float rv = -INFINITY;      /* this cell as an origin of END */
            int ro = 0x7fffffff, key = -1, wb = 0;
            if (valid) {
                const int wa = wordA[g], pos = wa & SH_SQP_POS_MASK, k = (wa >> SH_SQP_CAND_SHIFT) & SH_SQP_POS_MASK, st = pos + 1;
                const bool pos0 = wa & SH_SQP_POS0, pos1 = wa & SH_SQP_POS1, right = wa & SH_SQP_RIGHT;
                const int g1 = g >= 1 ? g - 1 : 0, g2 = g >= 2 ? g - 2 : 0, gr = g + 1 < NC ? g + 1 : g;
                key = k; wb = wordB[g];
                const float sv = pS[k], m0 = move0[k], from_start = sv + m0;
                const float pv = pP[g], mv = move[g];
                const float em = sq_emit(x, loc[g], scale[g], logsc[g], minscore);
                float v = pv + stay[g];
                const float s1 = pos0 ? from_start : pP[g1] + move[g1];
                const float s2 = ((pos1 ? sv : pP[g2]) + (pos1 ? m0 : move[g2])) - skip_pen;
                const float fs = from_start - local_pen * (float)pos;
                const float fb = pB[g1] + half_pen;
                const float mb = pP[gr] + back_pen;
                const float ec = (pv + mv) - local_pen * (float)(npos[k] - st);
                float bk = pB[g] + half_pen;
                if (VIT) {
                    if (s1 > v) v = s1;
                    if (!pos0) {
                        if (s2 > v) v = s2;
                        if (fs > v) v = fs;
                        if (fb > v) v = fb;
                    }
                    if (right) {
                        if (mb > bk) bk = mb;
                        if (ec > rv) { rv = ec; ro = st; }
                    }
                } else {
                    v = sh_lse(v, s1);
                    if (!pos0) {
                        v = sh_lse(v, s2);
                        v = sh_lse(v, fs);
                        v = sh_lse(v, fb);
                    }
                    if (right) {
                        bk = sh_lse(bk, mb);
                        rv = sq_lse0(rv, ec);
                    }
                }
                cP[g] = v + em;
                cB[g] = bk + em;
            }
            for (int d = 1; d < 64; d <<= 1) {          /* the pieces' END pairs: a lane takes in the lane d up where that is of its candidate */
                const float ov = __shfl_down(rv, d);
                const int ok = __shfl_down(key, d);
                const bool same = ln + d < 64 && ok == key;
                if (VIT) {
                    const int oo = __shfl_down(ro, d);
                    if (same && (ov > rv || (ov == rv && oo < ro))) { rv = ov; ro = oo; }
                } else if (same) rv = sq_lse0(rv, ov);
            }
            if (valid && (wb & SH_SQP_HEAD)) {
                const int pc = (t & 1) * NPC + (wb & SH_SQP_PIECE_MASK);
                part_v[pc] = rv; part_o[pc] = ro;
            }
        }
        x = xn;
        __syncthreads();
    }
    const float *f = rowP + (NS & 1) * NC;
    for (int k = tid; k < NK; k += SH_SQ_NTH) {
        const float xl = f[first[k] + npos[k] - 1], y = endv[k];
        a.score[pk.out + k] = VIT ? fmaxf(xl, y) : sh_lse(xl, y);
    }
}

#endif /* SH_SQUIG_PACK_H */
