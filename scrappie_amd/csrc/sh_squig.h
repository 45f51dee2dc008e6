/* sh_squig.h -- mapping of a raw signal to a predicted squiggle (decode.c:1016-1401, squiggle_match_viterbi / _forward): the
 * Viterbi or forward score of a local mapping, sample by sample, and the Viterbi path.
 *
 * States, as the reference numbers them: START (0), positions 1..npos, END (npos + 1) -- its nfstate = npos + 2 -- then
 * npos "back" states.  Back state k is entered from position state k + 2, emits with position k's parameters and leaves
 * to position state k + 2.  A score row holds START, the positions and the back states (2 npos + 1 floats: row index s
 * for state s <= npos, npos + 1 + k for back state k); END lives in a register of thread 0 (see "END" below).
 *
 * Work split: one workgroup of SH_SQ_NTH threads per read.  Samples are walked in order; within a sample every state
 * depends only on the previous sample's row, so 0-based position pos (state pos + 1, and back state pos with it: they
 * share the emission) belongs to thread pos % SH_SQ_NTH.  Two ping-pong rows, one barrier per sample.  The rows and
 * the per-position tables live in LDS while 36 npos + 88 bytes fit SH_SQ_LDS (npos <= SH_SQ_LDS_MAX_POS); beyond that
 * the rows are in device scratch and the tables are read where the host put them.  The two homes are two
 * instantiations, and a launch holds reads of one home only.
 *
 * Tables: scale = expf(log sd), move_pen and stay_pen (with their means for START and END) come from the host, computed
 * in C with the reference's expressions and summation order (sh_host.c: sh_squiggle_tables; libm's tanhf / logf /
 * log1pf / expf, as in the reference).  The device arithmetic of Viterbi is add, compare, one IEEE division and the
 * emission fmaxf(-minscore, loglaplace): util.h:75-77 subtracts the double constant M_LN2, so the reference evaluates
 * (double)(-fabsf(x - loc) / sc - logsc) - M_LN2 and rounds once; so does sq_emit.  With -ffp-contract=off Viterbi
 * scores and paths are bit-identical.  The comparisons are the reference's, all strict >, in its order:
 *   position  stay, step, skip, from START (- local_pen * destpos; 0-based destinations 1..npos-1), from back
 *   back      stay, from position state k + 2
 *   END       stay, step, skip, then origins origst = 1..npos-1 ascending with - local_pen * (npos - origst)
 * Afterwards the emission is added to position and back states, local_pen is subtracted from START and END.  Forward is
 * the same recursion with logsumexpf (util.h:162-164, sh_lse) in place of max.
 *
 * END: its maximum over all origins is a workgroup reduction per sample, and nothing but END reads END.  It trails the
 * recursion by one sample and adds no barrier: while iteration t computes row t + 1 from row t, every thread also forms
 * the END candidates of its own positions from the row-t values it has just read, keeps the first maximum (value,
 * origin) over its chunks, the wave reduces that with shuffles (ties go to the smaller origin = the reference's first
 * maximum) and lane 0 leaves the wave's pair in LDS slot t & 1.  Thread 0 reads row t's last two positions (END's step
 * and skip) in the same iteration.  After the sample's one barrier, at the top of iteration t + 1, thread 0 folds
 * stay, step, skip and the four pairs into END and writes END's source for sample t.  The slots are written again in
 * iteration t + 2, behind the barrier of t + 1.  The order of the forward sum is free.
 *
 * Traceback (Viterbi with path): per (sample, position) a 3-bit code for the position state -- 0 stay, 1 step, 2 skip,
 * 3 from START, 4 from back -- and one bit for its back state (1: entered from the position state): 4 bits per
 * position, kept as four bit planes per group of 64 positions (four wave ballots -> 8 words, two 16-byte stores by
 * lane 0): W = 8 ceil(npos / 64) words per sample.  END's source state is one int32 per sample after the codes
 * (it can be any origin); START always stays.  k_squig_walk walks a path back, one thread per read as k_map_walk does,
 * and applies the final recoding of decode.c:1210-1234 as it goes: START is only ever a prefix and END a suffix of a
 * path, so "-1 for leading START and trailing END samples, back states to their position, others state - 1" is a
 * function of the state alone.  All stores are plain vector stores.
 */
#ifndef SH_SQUIG_H
#define SH_SQUIG_H

#include "sh_map.h"     /* SH_MAP_BIG, sh_lse */

#define SH_SQ_NTH 256
#define SH_SQ_LDS 65536                                  /* dynamic LDS per workgroup at most */
#define SH_SQ_LDS_HEAD 16                                /* floats in front of the rows: the END pairs of 4 waves x 2 slots */
#define SH_SQ_LDS_MAX_POS ((SH_SQ_LDS / 4 - SH_SQ_LDS_HEAD - 6) / 9)      /* 1818: rows 2 (2 npos + 1) + tables 5 npos + 4 */
#define SH_SQ_MAX_POS (1 << 20)                          /* longest squiggle mapped (positions); longer: NAN and an error */

struct ShSquigRead {
    long long sig;      /* float offset of the read's first sample */
    long long tab;      /* float offset of its tables: loc[npos], scale[npos], logsc[npos], move_pen[npos + 2], stay_pen[npos + 2] */
    long long tb;       /* first traceback word (multiple of 4); -1: no traceback */
    long long scr;      /* float offset of the two score rows in device scratch; -1: in LDS */
    int nsample, npos;
    int ok;             /* 0: nothing to do (the host has set NAN) */
    int pad;
};

struct ShSquigArgs {
    const ShSquigRead *rd;
    const float *sig;
    const float *tab;
    unsigned *tb;
    float *scr;
    float *score;               /* [read] */
    int *final_state;           /* [read] Viterbi: npos or END (npos + 1) */
    float move_back_pen;        /* logf(prob_back) */
    float half_pen;             /* logf(0.5f): stay in back, move from back */
    float local_pen, skip_pen, minscore;
};

__host__ __device__ __forceinline__ long long sh_squig_words(int npos) { return 8ll * ((npos + 63) / 64); }

/* fmaxf(-minscore, loglaplace(x, loc, sc, logsc)), util.h:75-77 with its one rounding from double */
__device__ __forceinline__ float sq_emit(float x, float loc, float sc, float logsc, float minscore) {
    const float f = __fdiv_rn(-fabsf(x - loc), sc) - logsc;
    return fmaxf(-minscore, (float)((double)f - 0.693147180559945309417232121458176568));
}

/* logsumexpf with -inf as the empty sum (the END partial sums start empty) */
__device__ __forceinline__ float sq_lse0(float x, float y) {
    if (x == -INFINITY) return y;
    if (y == -INFINITY) return x;
    return sh_lse(x, y);
}

template <bool VIT, bool LDS>
__global__ __launch_bounds__(SH_SQ_NTH) void k_squig(ShSquigArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_sq_lds[];
    const ShSquigRead r = a.rd[blockIdx.x];
    if (!r.ok) return;
    const int tid = threadIdx.x, NP = r.npos, NS = r.nsample, RW = 2 * NP + 1, BK = NP + 1, END = NP + 1;
    float *const part_v = sh_sq_lds;                         /* [slot][wave] */
    int *const part_o = (int *)(sh_sq_lds + 8);
    float *const buf0 = LDS ? sh_sq_lds + SH_SQ_LDS_HEAD : a.scr + r.scr;
    float *const buf1 = buf0 + RW;
    const float *const gtab = a.tab + r.tab;
    float *const ltab = sh_sq_lds + SH_SQ_LDS_HEAD + 2 * RW;
    if (LDS)
        for (int i = tid; i < 5 * NP + 4; i += SH_SQ_NTH) ltab[i] = gtab[i];
    const float *const tab = LDS ? (const float *)ltab : gtab;
    const float *const loc = tab, *const scale = tab + NP, *const logsc = tab + 2 * NP, *const move = tab + 3 * NP, *const stay = tab + 4 * NP + 2;
    for (int i = tid; i < RW; i += SH_SQ_NTH) { buf0[i] = i == 0 ? 0.0f : -SH_MAP_BIG; buf1[i] = -SH_MAP_BIG; }
    const float *const sig = a.sig + r.sig;
    const float local_pen = a.local_pen, skip_pen = a.skip_pen, minscore = a.minscore, back_pen = a.move_back_pen, half_pen = a.half_pen;
    const bool want_tb = VIT && r.tb >= 0;
    const long long W = sh_squig_words(NP);
    unsigned *const tbw = want_tb ? a.tb + r.tb : nullptr;
    int *const tbe = want_tb ? (int *)(tbw + (long long)NS * W) : nullptr;
    const int nch = (NP + SH_SQ_NTH - 1) / SH_SQ_NTH, ngrp = (NP + 63) / 64;
    const int wv = tid >> 6, ln = tid & 63;
    float endv = -SH_MAP_BIG, e_step = 0.0f, e_skip = 0.0f;      /* thread 0: END of the current row; its step and skip candidates */
    float x = sig[0];
    __syncthreads();
    for (int t = 0; t <= NS; t++) {
        const float *p = (t & 1) ? buf1 : buf0;
        float *c = (t & 1) ? buf0 : buf1;
        if (tid == 0) {
            if (t > 0) {                 /* END of row t from row t - 1: stay, step, skip, then the origins' first maximum */
                const int sl = (t - 1) & 1;
                float e = endv + stay[END];
                int src = END;
                if (VIT) {
                    if (e_step > e) { e = e_step; src = NP; }
                    if (e_skip > e) { e = e_skip; src = NP - 1; }
                    float bv = part_v[sl * 4];
                    int bo = part_o[sl * 4];
                    for (int w = 1; w < 4; w++) {
                        const float ov = part_v[sl * 4 + w];
                        const int oo = part_o[sl * 4 + w];
                        if (ov > bv || (ov == bv && oo < bo)) { bv = ov; bo = oo; }
                    }
                    if (bv > e) { e = bv; src = bo; }
                    if (want_tb) tbe[t - 1] = src;
                } else {
                    e = sh_lse(e, e_step);
                    e = sh_lse(e, e_skip);
                    float acc = part_v[sl * 4];
                    for (int w = 1; w < 4; w++) acc = sq_lse0(acc, part_v[sl * 4 + w]);
                    if (acc != -INFINITY) e = sh_lse(e, acc);
                }
                endv = e - local_pen;
            }
            if (t < NS) {
                e_step = p[NP] + move[NP];
                e_skip = (p[NP - 1] + move[NP - 1]) - skip_pen;
            }
        }
        if (t == NS) break;
        const float xn = sig[t + 1 < NS ? t + 1 : t];      /* the next sample, asked for before the barrier */
        const float from_start = p[0] + move[0];
        float bestv = -INFINITY;
        int besto = 0x7fffffff;
        for (int ch = 0; ch < nch; ch++) {
            const int pos = ch * SH_SQ_NTH + tid, st = pos + 1;
            const bool valid = pos < NP;
            int code = 0, bbit = 0;
            if (valid) {
                const float pv = p[st];
                const float em = sq_emit(x, loc[pos], scale[pos], logsc[pos], minscore);
                float v = pv + stay[st];
                const float s1 = p[st - 1] + move[st - 1];
                float bk = p[BK + pos] + half_pen;
                if (VIT) {
                    if (s1 > v) { v = s1; code = 1; }
                    if (st >= 2) { const float s2 = (p[st - 2] + move[st - 2]) - skip_pen; if (s2 > v) { v = s2; code = 2; } }
                    if (pos >= 1) {
                        const float fs = from_start - local_pen * (float)pos;
                        if (fs > v) { v = fs; code = 3; }
                        const float fb = p[BK + pos - 1] + half_pen;
                        if (fb > v) { v = fb; code = 4; }
                    }
                    if (pos <= NP - 2) { const float mb = p[pos + 2] + back_pen; if (mb > bk) { bk = mb; bbit = 1; } }
                    if (pos <= NP - 2) {             /* origin st of END: 1..npos-1 */
                        const float ec = (pv + move[st]) - local_pen * (float)(NP - st);
                        if (ec > bestv) { bestv = ec; besto = st; }
                    }
                } else {
                    v = sh_lse(v, s1);
                    if (st >= 2) v = sh_lse(v, (p[st - 2] + move[st - 2]) - skip_pen);
                    if (pos >= 1) {
                        v = sh_lse(v, from_start - local_pen * (float)pos);
                        v = sh_lse(v, p[BK + pos - 1] + half_pen);
                    }
                    if (pos <= NP - 2) bk = sh_lse(bk, p[pos + 2] + back_pen);
                    if (pos <= NP - 2) bestv = sq_lse0(bestv, (pv + move[st]) - local_pen * (float)(NP - st));
                }
                c[st] = v + em;
                c[BK + pos] = bk + em;
            }
            if (want_tb) {
                const unsigned long long b0 = __ballot(valid && (code & 1)), b1 = __ballot(valid && (code & 2)),
                                         b2 = __ballot(valid && (code & 4)), b3 = __ballot(valid && bbit);
                const int g = ch * (SH_SQ_NTH / 64) + wv;
                if (ln == 0 && g < ngrp) {
                    uint4 *dst = (uint4 *)(tbw + (long long)t * W + (long long)g * 8);
                    dst[0] = make_uint4((unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1, (unsigned)(b1 >> 32));
                    dst[1] = make_uint4((unsigned)b2, (unsigned)(b2 >> 32), (unsigned)b3, (unsigned)(b3 >> 32));
                }
            }
        }
        if (tid == 0) c[0] = (p[0] + stay[0]) - local_pen;
        for (int d = 32; d >= 1; d >>= 1) {          /* the wave's END pair */
            const float ov = __shfl_xor(bestv, d);
            if (VIT) {
                const int oo = __shfl_xor(besto, d);
                if (ov > bestv || (ov == bestv && oo < besto)) { bestv = ov; besto = oo; }
            } else bestv = sq_lse0(bestv, ov);
        }
        if (ln == 0) { part_v[(t & 1) * 4 + wv] = bestv; part_o[(t & 1) * 4 + wv] = besto; }
        x = xn;
        __syncthreads();
    }
    if (tid == 0) {
        const float *f = (NS & 1) ? buf1 : buf0;
        const float xl = f[NP], y = endv;
        a.score[blockIdx.x] = VIT ? fmaxf(xl, y) : sh_lse(xl, y);
        if (VIT && a.final_state) a.final_state[blockIdx.x] = (xl > y) ? NP : END;
    }
}

/* decode.c:1204-1234, one thread per read: path[sample] in 0..npos-1, -1 in START and END */
__global__ __launch_bounds__(64) void k_squig_walk(const ShSquigRead *__restrict__ rd, int n, const unsigned *__restrict__ tb,
                                                   const int *__restrict__ final_state, const long long *__restrict__ path_off,
                                                   int *__restrict__ path) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShSquigRead r = rd[i];
    if (!r.ok || r.tb < 0 || path_off[i] < 0) return;
    const int NP = r.npos, NS = r.nsample, NF = NP + 2;
    const long long W = sh_squig_words(NP);
    const unsigned *w = tb + r.tb;
    const int *we = (const int *)(w + (long long)NS * W);
    int *out = path + path_off[i];
    int st = final_state[i];
    for (int t = NS - 1; t >= 0; t--) {
        out[t] = (st == 0 || st == NF - 1) ? -1 : (st >= NF ? st - NF : st - 1);
        if (t == 0) break;
        int prev;
        if (st == 0) prev = 0;
        else if (st == NF - 1) prev = we[t];
        else {
            const int pos = st >= NF ? st - NF : st - 1;
            const unsigned *g = w + (long long)t * W + (long long)(pos >> 6) * 8 + ((pos & 63) >> 5);
            const int sh = pos & 31;
            if (st >= NF) prev = ((g[6] >> sh) & 1u) ? pos + 2 : st;
            else {
                const int code = (int)(((g[0] >> sh) & 1u) | (((g[2] >> sh) & 1u) << 1) | (((g[4] >> sh) & 1u) << 2));
                prev = code == 0 ? st : code == 1 ? st - 1 : code == 2 ? st - 2 : code == 3 ? 0 : NF + st - 2;
            }
        }
        st = prev;
    }
}

#endif /* SH_SQUIG_H */
