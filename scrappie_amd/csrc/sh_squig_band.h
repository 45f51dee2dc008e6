/* sh_squig_band.h -- the recursion of sh_squig.h inside a band: per read one width WD and, per sample t, the first position
 * low[t] (non-decreasing, 0 <= low[t] <= npos - 1) of the band [low[t], min(low[t] + WD, npos)).  The recursion, its candidates,
 * their order, the strict >, the emission and the END reduction are those of k_squig; the one change: once the row of sample t is
 * complete, every position state and every back state outside sample t's band holds -SH_MAP_BIG (what the rows start with).
 * START and END are never masked.  A band of low = 0 and WD = npos is k_squig bit for bit, and so is any band that contains the
 * unbanded Viterbi path (the first maximum stays the first maximum when other candidates only become smaller).
 *
 * Rows, band-relative: a row holds START, then WD position cells, then WD back cells (2 WD + 1 floats); cell j of the row of
 * sample t is position low[t] + j.  Masked cells are not stored: a read of position q from the previous row (rdst, rdbk) is
 * predicated on lo_p <= q < hi_p, the previous sample's band: row[1 + q - lo_p] inside it and the constant -SH_MAP_BIG outside,
 * never a load from outside the row.  Cells whose position would be >= npos are neither written nor read.  The row before the
 * first sample has an empty band (lo_p = hi_p = 0): START = 0 and the constant everywhere else.  Band-relative rather than
 * circular (pos % WD) because a band may jump any distance between two samples: here a jump costs nothing and needs no
 * clearing of cells that left the band, and the predicate is two compares on values every thread already holds.  What it gives
 * up: a position changes thread as the band slides, so its table entries are loaded again for every sample.
 *
 * Homes: two rows and the END pairs in LDS while (SH_SQ_LDS_HEAD + 2 (2 WD + 1)) floats fit SH_SQ_LDS (WD <= SH_SQB_LDS_MAX_W,
 * whatever npos is), in device scratch beyond; two instantiations, a launch holds one home.  The tables of a long squiggle
 * (5 npos + 4 floats) do not fit LDS beside the rows: both homes read them from device memory where the host put them --
 * neighbouring lanes read neighbouring floats, a band's window of them is a few KB that L1 and L2 keep, and the same addresses
 * come back one sample later.  Workgroup: SH_SQ_NTH threads whatever the width; a narrow band leaves waves idle at the barrier
 * and keeps the four END slots and the chunk arithmetic those of k_squig.
 *
 * END trails by one sample as in k_squig: iteration t forms the END candidates of row t (the previous row, band [lo_p, hi_p))
 * while it computes row t + 1 from it.  A thread sees the previous row at its own positions low[t] + j; the positions of the
 * previous band that sample t's band has left behind ([lo_p, min(low[t], hi_p)), all smaller than the thread's own) are read in a
 * short loop first, so origins still come in ascending order per thread.  Origins outside the previous band are left out: their
 * candidate is -SH_MAP_BIG exactly (1e30 absorbs every penalty), END itself never falls below that, and strict > never takes it.
 *
 * Traceback: the 4 bits per cell of k_squig as four ballot planes per group of 64 CELLS: 8 ceil(WD / 64) words per sample,
 * then END's source, one int32 per sample.  k_squig_band_walk finds a position's cell with low[] (pos - low[t]).  A finite best
 * path never passes through a masked cell.  A final score below -SH_MAP_BIG / 2 means the band admits no path: the kernel leaves
 * final_state = -1, the walk skips the read and the host answers NAN.  All stores are plain vector stores.
 */
#ifndef SH_SQUIG_BAND_H
#define SH_SQUIG_BAND_H

#include "sh_squig.h"   /* sq_emit, sq_lse0, sh_squig_words, SH_SQ_* */

#define SH_SQB_LDS_MAX_W ((SH_SQ_LDS / 4 - SH_SQ_LDS_HEAD - 2) / 4)       /* rows 2 (2 WD + 1) floats behind the head */

struct ShSquigBandRead {
    long long sig;      /* float offset of the read's first sample */
    long long tab;      /* float offset of its tables, as ShSquigRead::tab */
    long long tb;       /* first traceback word (multiple of 4); -1: no traceback */
    long long scr;      /* float offset of the two score rows in device scratch; -1: in LDS */
    const int *low;     /* low[nsample], on the device (uploaded behind the signals) */
    int nsample, npos;
    int width;
    int ok;             /* 0: nothing to do (the host has set NAN) */
};

struct ShSquigBandArgs {
    const ShSquigBandRead *rd;
    const float *sig;
    const float *tab;
    unsigned *tb;
    float *scr;
    float *score;               /* [read] */
    int *final_state;           /* [read] Viterbi: npos or END (npos + 1); -1: the band admits no path */
    float move_back_pen, half_pen;
    float local_pen, skip_pen, minscore;
};

template <bool VIT, bool LDS>
__global__ __launch_bounds__(SH_SQ_NTH) void k_squig_band(ShSquigBandArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_sqb_lds[];
    const ShSquigBandRead r = a.rd[blockIdx.x];
    if (!r.ok) return;
    const int tid = threadIdx.x, NP = r.npos, NS = r.nsample, WD = r.width, RW = 2 * WD + 1, BK = WD + 1, END = NP + 1;
    float *const part_v = sh_sqb_lds;                        /* [slot][wave] */
    int *const part_o = (int *)(sh_sqb_lds + 8);
    float *const buf0 = LDS ? sh_sqb_lds + SH_SQ_LDS_HEAD : a.scr + r.scr;
    float *const buf1 = buf0 + RW;
    const float *const tab = a.tab + r.tab;
    const float *const loc = tab, *const scale = tab + NP, *const logsc = tab + 2 * NP, *const move = tab + 3 * NP, *const stay = tab + 4 * NP + 2;
    for (int i = tid; i < RW; i += SH_SQ_NTH) { buf0[i] = i == 0 ? 0.0f : -SH_MAP_BIG; buf1[i] = -SH_MAP_BIG; }
    const float *const sig = a.sig + r.sig;
    const int *const low = r.low;
    const float local_pen = a.local_pen, skip_pen = a.skip_pen, minscore = a.minscore, back_pen = a.move_back_pen, half_pen = a.half_pen;
    const bool want_tb = VIT && r.tb >= 0;
    const long long W = sh_squig_words(WD);
    unsigned *const tbw = want_tb ? a.tb + r.tb : nullptr;
    int *const tbe = want_tb ? (int *)(tbw + (long long)NS * W) : nullptr;
    const int nch = (WD + SH_SQ_NTH - 1) / SH_SQ_NTH, ngrp = (WD + 63) / 64;
    const int wv = tid >> 6, ln = tid & 63;
    float endv = -SH_MAP_BIG, e_step = 0.0f, e_skip = 0.0f;
    float x = sig[0];
    int lo_p = 0, hi_p = 0;                                  /* the band of row p: none before the first sample */
    int lo_c = low[0];
    __syncthreads();
    for (int t = 0; t <= NS; t++) {
        const float *p = (t & 1) ? buf1 : buf0;
        float *c = (t & 1) ? buf0 : buf1;
        /* state s (0: START, else position s - 1) and back state q of row p; outside its band the constant */
        auto rdst = [&](int s) -> float {
            if (s == 0) return p[0];
            const int q = s - 1;
            return (q >= lo_p && q < hi_p) ? p[1 + (q - lo_p)] : -SH_MAP_BIG;
        };
        auto rdbk = [&](int q) -> float { return (q >= lo_p && q < hi_p) ? p[BK + (q - lo_p)] : -SH_MAP_BIG; };
        if (tid == 0) {
            if (t > 0) {                 /* END of row t from row t - 1, as k_squig */
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
                e_step = rdst(NP) + move[NP];
                e_skip = (rdst(NP - 1) + move[NP - 1]) - skip_pen;
            }
        }
        if (t == NS) break;
        const int hi_c = min(lo_c + WD, NP);
        const float xn = sig[t + 1 < NS ? t + 1 : t];       /* the next sample and its band, asked for before the barrier */
        const int lo_n = low[t + 1 < NS ? t + 1 : t];
        const float from_start = p[0] + move[0];
        float bestv = -INFINITY;
        int besto = 0x7fffffff;
        for (int q = lo_p + tid; q < min(lo_c, hi_p); q += SH_SQ_NTH) {      /* END origins the band has left behind */
            const int st = q + 1;
            if (q <= NP - 2) {
                const float ec = (p[1 + (q - lo_p)] + move[st]) - local_pen * (float)(NP - st);
                if (VIT) { if (ec > bestv) { bestv = ec; besto = st; } }
                else bestv = sq_lse0(bestv, ec);
            }
        }
        for (int ch = 0; ch < nch; ch++) {
            const int j = ch * SH_SQ_NTH + tid, pos = lo_c + j, st = pos + 1;
            const bool valid = j < WD && pos < hi_c;
            int code = 0, bbit = 0;
            if (valid) {
                const bool inb = pos >= lo_p && pos < hi_p;
                const float pv = inb ? p[1 + (pos - lo_p)] : -SH_MAP_BIG;
                const float em = sq_emit(x, loc[pos], scale[pos], logsc[pos], minscore);
                float v = pv + stay[st];
                const float s1 = rdst(st - 1) + move[st - 1];
                float bk = rdbk(pos) + half_pen;
                if (VIT) {
                    if (s1 > v) { v = s1; code = 1; }
                    if (st >= 2) { const float s2 = (rdst(st - 2) + move[st - 2]) - skip_pen; if (s2 > v) { v = s2; code = 2; } }
                    if (pos >= 1) {
                        const float fs = from_start - local_pen * (float)pos;
                        if (fs > v) { v = fs; code = 3; }
                        const float fb = rdbk(pos - 1) + half_pen;
                        if (fb > v) { v = fb; code = 4; }
                    }
                    if (pos <= NP - 2) { const float mb = rdst(pos + 2) + back_pen; if (mb > bk) { bk = mb; bbit = 1; } }
                    if (inb && pos <= NP - 2) {      /* origin st of END: 1..npos-1 */
                        const float ec = (pv + move[st]) - local_pen * (float)(NP - st);
                        if (ec > bestv) { bestv = ec; besto = st; }
                    }
                } else {
                    v = sh_lse(v, s1);
                    if (st >= 2) v = sh_lse(v, (rdst(st - 2) + move[st - 2]) - skip_pen);
                    if (pos >= 1) {
                        v = sh_lse(v, from_start - local_pen * (float)pos);
                        v = sh_lse(v, rdbk(pos - 1) + half_pen);
                    }
                    if (pos <= NP - 2) bk = sh_lse(bk, rdst(pos + 2) + back_pen);
                    if (inb && pos <= NP - 2) bestv = sq_lse0(bestv, (pv + move[st]) - local_pen * (float)(NP - st));
                }
                c[1 + j] = v + em;
                c[BK + j] = bk + em;
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
        lo_p = lo_c; hi_p = hi_c; lo_c = lo_n;
        __syncthreads();
    }
    if (tid == 0) {
        const float *f = (NS & 1) ? buf1 : buf0;
        const float xl = (NP - 1 >= lo_p && NP - 1 < hi_p) ? f[1 + (NP - 1 - lo_p)] : -SH_MAP_BIG, y = endv;
        const float sc = VIT ? fmaxf(xl, y) : sh_lse(xl, y);
        a.score[blockIdx.x] = sc;
        if (VIT && a.final_state) a.final_state[blockIdx.x] = sc < -SH_MAP_BIG / 2 ? -1 : (xl > y) ? NP : END;
    }
}

/* k_squig_walk over band-relative codes: one thread per read; the cell of position pos at sample t is pos - low[t] */
__global__ __launch_bounds__(64) void k_squig_band_walk(const ShSquigBandRead *__restrict__ rd, int n, const unsigned *__restrict__ tb,
                                                        const int *__restrict__ final_state, const long long *__restrict__ path_off,
                                                        int *__restrict__ path) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShSquigBandRead r = rd[i];
    if (!r.ok || r.tb < 0 || path_off[i] < 0) return;
    int st = final_state[i];
    if (st < 0) return;                              /* no path */
    const int NP = r.npos, NS = r.nsample, NF = NP + 2, WD = r.width;
    const long long W = sh_squig_words(WD);
    const unsigned *w = tb + r.tb;
    const int *we = (const int *)(w + (long long)NS * W);
    const int *low = r.low;
    int *out = path + path_off[i];
    for (int t = NS - 1; t >= 0; t--) {
        out[t] = (st == 0 || st == NF - 1) ? -1 : (st >= NF ? st - NF : st - 1);
        if (t == 0) break;
        int prev;
        if (st == 0) prev = 0;
        else if (st == NF - 1) prev = we[t];
        else {
            const int pos = st >= NF ? st - NF : st - 1, j = pos - low[t];
            if ((unsigned)j >= (unsigned)WD) {       /* (a finite path stays inside the band; never read outside the codes) */
                for (int u = t - 1; u >= 0; u--) out[u] = -1;
                break;
            }
            const unsigned *g = w + (long long)t * W + (long long)(j >> 6) * 8 + ((j & 63) >> 5);
            const int sh = j & 31;
            if (st >= NF) prev = ((g[6] >> sh) & 1u) ? pos + 2 : st;
            else {
                const int code = (int)(((g[0] >> sh) & 1u) | (((g[2] >> sh) & 1u) << 1) | (((g[4] >> sh) & 1u) << 2));
                prev = code == 0 ? st : code == 1 ? st - 1 : code == 2 ? st - 2 : code == 3 ? 0 : NF + st - 2;
            }
        }
        st = prev;
    }
}

#endif /* SH_SQUIG_BAND_H */
