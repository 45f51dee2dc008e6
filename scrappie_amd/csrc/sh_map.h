/* sh_map.h -- block-based mapping of a transducer posterior to a sequence (decode.c:1420-1964): the Viterbi and forward
 * scores of a local-global alignment, full or banded, and the Viterbi path.
 *
 * States are seq[0..L), then START (L), then END (L+1); the stay row is the posterior's last row.  One template covers the
 * four recursions ({Viterbi, forward} x {full, banded}) and both posterior layouts:
 *   dense  a read's posterior as the reference holds it: row blk at post + blk * pstride, already log (the per-read surface)
 *   tiled  the engine's S1 output, E + sums: the chunk layout k_gather_read decodes (sh_crf.h); an entry is finalised with the
 *          same fin_post(v, d_rcp(sum), min_prob, 1 - min_prob, 1) call, so the DP sees the bits scrappie_hip_posterior returns
 *
 * Work split: one workgroup of SH_MAP_NTH threads per read.  Blocks are walked in order; within a block every position is
 * independent given the previous block's row, so position pos belongs to thread pos % SH_MAP_NTH.  The two score rows
 * (pscore, cscore) are ping-pong buffers of L + 2 floats: one barrier per block.  They live in LDS, beside the state codes
 * (loaded once), while 12 L + 16 bytes fit SH_MAP_LDS; longer sequences keep them in device scratch (the codes are then read
 * from the read's own array).  The two homes are two instantiations, and a launch holds reads of one home only.  Each read gathers only its L state entries and the stay entry of a block: a row of the
 * tiled posterior is 16-byte pieces spread across each 1 KiB chunk, and a sequence touches a few hundred of 1025 states.
 *
 * The banded forms keep the reference's buffers literally: both rows start at -1e30 and are never cleared, so a cell outside
 * the current band keeps what the same buffer held two blocks earlier; block 0 assigns cscore[1] and cscore[2] from seq[1]
 * and seq[2]; seq -> END reads pscore[L-1] whether or not it is in the band.
 *
 * Viterbi arithmetic is the reference's operation for operation ((p - stay_pen) + lp, strict > in the order stay, step,
 * skip, START -> 0; END: stay, then seq -> END), and the build has -ffp-contract=off: scores and paths are bit-identical.
 * Forward uses logsumexpf as util.h:162-164 with the accurate device expf / log1pf.  The unbanded cell is sh_map_cell, which
 * k_map_pack (sh_map_pack.h: several candidates of one read in one workgroup) goes through as well.
 *
 * Traceback (unbanded Viterbi): a 2-bit move code per (block, position) -- 0 stay, 1 step, 2 skip, 3 from START -- packed 16
 * to a 32-bit word from two wave ballots and written as one 16-byte store per wave and block; W = 4 ceil(L / 64) words per
 * block.  END's source (stay or seq[L-1]) is one bit per block after the codes.  START's source is always START.
 * k_map_walk walks a path back, one thread per read, as k_backtrace does.
 */
#ifndef SH_MAP_H
#define SH_MAP_H

#define SH_MAP_NTH 256
#define SH_MAP_LDS 65536          /* dynamic LDS per workgroup at most (the default limit: no function attribute needed); sh_internal.h repeats it for the host C */
#define SH_MAP_MAX_SEQ 65536      /* longest sequence mapped (states); longer: NAN and an error */
#define SH_MAP_BIG 1.e30f         /* decode.c:8 */

struct ShMapRead {
    long long post;     /* dense: float offset of the read's row 0; tiled: the read's first column block */
    long long tb;       /* first traceback word (multiple of 4); -1: no traceback */
    long long scr;      /* float offset of the two score rows in device scratch; -1: in LDS */
    long long seq;      /* offset of the read's state codes */
    long long band;     /* offset of poslow (nblock int32) and poshigh (the next nblock); -1: unbanded */
    int nblock, seqlen;
    int lane;           /* tiled: the read's lane in its tile (0..15) */
    int ok;             /* 0: nothing to do (the host has set NAN) */
};

struct ShMapArgs {
    const ShMapRead *rd;
    const float *post;          /* dense posterior */
    const float *E, *sums;      /* tiled posterior */
    long long pstride;          /* dense: floats per row */
    int nr;                     /* states, stay included */
    int nchunk;                 /* tiled: chunks of 16 states per column block */
    float min_prob;             /* tiled: fin_post's floor */
    float stay_pen, skip_pen, local_pen;
    const int *seq;
    const int *band;
    unsigned *tb;
    float *scr;
    float *score;               /* [read] */
    int *final_state;           /* [read] Viterbi: L - 1 or END */
};

__device__ __forceinline__ int sh_map_words(int L) { return 4 * ((L + 63) / 64); }

/* util.h:162-164 */
__device__ __forceinline__ float sh_lse(float x, float y) { return fmaxf(x, y) + log1pf(expf(-fabsf(x - y))); }

template <bool TILED> struct ShMapPost;
template <> struct ShMapPost<false> {
    const float *row;
    __device__ __forceinline__ void block(const ShMapArgs &a, const ShMapRead &r, int blk) { row = a.post + r.post + (long long)blk * a.pstride; }
    __device__ __forceinline__ float operator()(int s) const { return row[s]; }
};
template <> struct ShMapPost<true> {
    const float *col;
    float rcp, mp, mpm1;
    __device__ __forceinline__ void block(const ShMapArgs &a, const ShMapRead &r, int blk) {
        const long long cb = r.post + blk;
        col = a.E + cb * a.nchunk * 256 + r.lane * 4;
        rcp = d_rcp(a.sums[cb * 16 + r.lane]);
        mp = a.min_prob; mpm1 = 1.0f - a.min_prob;
    }
    __device__ __forceinline__ float operator()(int s) const {
        return fin_post(col[(s >> 4) * 256 + ((s >> 2) & 3) * 64 + (s & 3)], rcp, mp, mpm1, 1);
    }
};

__device__ __forceinline__ unsigned sh_spread16(unsigned x) {
    x &= 0xffffu;
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

/* One cell of the unbanded recursion (decode.c:1448-1478, :1580-1600), shared by k_map and k_map_pack (sh_map_pack.h): p the
 * previous block's row, i the cell in it, le the cell's posterior entry, lps the stay entry.  pos: the cell's position in its
 * sequence, of which only 0, 1 and "2 or more" matter: from 1 on it has a left neighbour (i - 1), from 2 on two of them (i - 2),
 * and position 0 reads START at p[start].
 * The reference's expressions in its order -- stay, step, skip, START -- with strict > (code: the move taken) or sh_lse.  Row: a pointer, or
 * what answers p[i] as one does (k_map_edits_rows reads the row under a band: ShMapEditsRow, sh_map_edits.h). */
template <bool VIT, class Row>
__device__ __forceinline__ float sh_map_cell(const Row p, int i, int start, int pos, float le, float lps, float stay_pen, float skip_pen,
                                             int &code) {
    float v = (p[i] - stay_pen) + lps;
    if (VIT) {
        int c = 0;
        if (pos >= 1) { const float st = p[i - 1] + le; if (st > v) { v = st; c = 1; } }
        if (pos >= 2) { const float sk = (p[i - 2] - skip_pen) + le; if (sk > v) { v = sk; c = 2; } }
        if (pos == 0) { const float fs = p[start] + le; if (fs > v) { v = fs; c = 3; } }
        code = c;
    } else {
        if (pos >= 1) v = sh_lse(v, p[i - 1] + le);
        if (pos >= 2) v = sh_lse(v, (p[i - 2] - skip_pen) + le);
        if (pos == 0) v = sh_lse(v, p[start] + le);
    }
    return v;
}

/* LDS: the score rows and the codes in LDS (the launch holds only reads with scr < 0); else in device scratch.  The two
 * homes are separate instantiations: a pointer never selects between LDS and global memory at run time. */
template <bool VIT, bool BAND, bool TILED, bool LDS>
__global__ __launch_bounds__(SH_MAP_NTH) void k_map(ShMapArgs a) {
    extern __shared__ float sh_map_lds[];
    const ShMapRead r = a.rd[blockIdx.x];
    if (!r.ok) return;
    const int tid = threadIdx.x, L = r.seqlen, NB = r.nblock, NSQ = L + 2, START = L, END = L + 1, STAY = a.nr - 1;
    const float stay_pen = a.stay_pen, skip_pen = a.skip_pen, local_pen = a.local_pen;
    float *const buf0 = LDS ? sh_map_lds : a.scr + r.scr;
    float *const buf1 = buf0 + NSQ;
    int *const lds_seq = (int *)(sh_map_lds + 2 * NSQ);
    if (LDS)
        for (int i = tid; i < L; i += SH_MAP_NTH) lds_seq[i] = a.seq[r.seq + i];
    const int *const sq = LDS ? (const int *)lds_seq : a.seq + r.seq;
    for (int i = tid; i < NSQ; i += SH_MAP_NTH) { buf0[i] = i == START ? 0.0f : -SH_MAP_BIG; buf1[i] = -SH_MAP_BIG; }
    const int *lo = BAND ? a.band + r.band : nullptr, *hi = BAND ? lo + NB : nullptr;
    const bool want_tb = VIT && !BAND && r.tb >= 0;
    const int W = sh_map_words(L);
    unsigned *tbw = want_tb ? a.tb + r.tb : nullptr;
    unsigned endbits = 0;
    const int nch = (L + SH_MAP_NTH - 1) / SH_MAP_NTH;
    __syncthreads();
    ShMapPost<TILED> lp;
    for (int blk = 0; blk < NB; blk++) {
        const float *p = (blk & 1) ? buf1 : buf0;
        float *c = (blk & 1) ? buf0 : buf1;
        lp.block(a, r, blk);
        const float lps = lp(STAY);
        int lob = 0, hib = 0, s0 = 0, s1 = 0, k0 = 0, k1 = 0, hip = 0;
        if (BAND) {
            lob = lo[blk]; hib = hi[blk];
            if (blk > 0) {               /* decode.c:1785-1806 */
                const int lop = lo[blk - 1];
                hip = hi[blk - 1];
                s0 = max(lob, lop + 1); s1 = min(hib, hip + 1);
                k0 = max(lob, lop + 2); k1 = min(hib, hip + 2);
            }
        }
        for (int ch = 0; ch < nch; ch++) {
            const int pos = ch * SH_MAP_NTH + tid;
            const bool valid = pos < L;
            int code = 0;
            if (valid) {
                float v;
                if (!BAND) {
                    const float le = lp(sq[pos]);
                    v = sh_map_cell<VIT>(p, pos, START, pos, le, lps, stay_pen, skip_pen, code);
                } else if (blk == 0) {           /* decode.c:1744-1769 */
                    v = c[pos];
                    if (pos <= 2) {
                        const float le = lp(sq[pos]);
                        if (pos == 0) {
                            const float x = (p[0] + lps) - stay_pen;
                            v = VIT ? fmaxf(v, x) : sh_lse(v, x);
                            const float fs = p[START] + le;
                            v = VIT ? fmaxf(v, fs) : sh_lse(v, fs);
                        } else if (pos == 1) {
                            if (hib > 0) v = le;
                        } else {
                            if (hib > 1) v = le - skip_pen;
                        }
                    }
                } else {
                    v = c[pos];
                    if (lob <= pos && pos < hip) v = (p[pos] - stay_pen) + lps;
                    const bool in_step = s0 <= pos && pos < s1, in_skip = k0 <= pos && pos < k1, in_start = pos == 0 && lob == 0;
                    if (in_step || in_skip || in_start) {
                        const float le = lp(sq[pos]);
                        if (in_step) { const float st = p[pos - 1] + le; v = VIT ? fmaxf(st, v) : sh_lse(st, v); }
                        if (in_skip) { const float sk = (p[pos - 2] - skip_pen) + le; v = VIT ? fmaxf(sk, v) : sh_lse(sk, v); }
                        if (in_start) { const float fs = p[START] + le; v = VIT ? fmaxf(v, fs) : sh_lse(v, fs); }
                    }
                }
                c[pos] = v;
            }
            if (want_tb) {
                const unsigned long long b0 = __ballot(valid && (code & 1)), b1 = __ballot(valid && (code & 2));
                const int wv = tid >> 6, w0 = ch * (SH_MAP_NTH / 16) + wv * 4;
                if ((tid & 63) == 0 && w0 < W) {
                    uint4 q;
                    q.x = sh_spread16((unsigned)b0) | (sh_spread16((unsigned)b1) << 1);
                    q.y = sh_spread16((unsigned)(b0 >> 16)) | (sh_spread16((unsigned)(b1 >> 16)) << 1);
                    q.z = sh_spread16((unsigned)(b0 >> 32)) | (sh_spread16((unsigned)(b1 >> 32)) << 1);
                    q.w = sh_spread16((unsigned)(b0 >> 48)) | (sh_spread16((unsigned)(b1 >> 48)) << 1);
                    *(uint4 *)(tbw + (long long)blk * W + w0) = q;
                }
            }
        }
        if (tid == 0) {
            const float ls = VIT ? fmaxf(-local_pen, lps) : sh_lse(-local_pen, lps);
            c[START] = p[START] + ls;
            float e = p[END] + ls;
            const float ex = p[L - 1] - local_pen;
            if (BAND && blk == 0) {
                const float se = p[START] - local_pen;
                e = VIT ? fmaxf(e, se) : sh_lse(e, se);
            }
            if (VIT && !BAND) {
                if (ex > e) { e = ex; endbits |= 1u << (blk & 31); }
            } else {
                e = VIT ? fmaxf(e, ex) : sh_lse(e, ex);
            }
            c[END] = e;
            if (want_tb && ((blk & 31) == 31 || blk == NB - 1)) { tbw[(long long)NB * W + (blk >> 5)] = endbits; endbits = 0; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float *f = (NB & 1) ? buf1 : buf0;
        const float x = f[L - 1], y = f[END];
        a.score[blockIdx.x] = VIT ? fmaxf(x, y) : sh_lse(x, y);
        if (VIT && a.final_state) a.final_state[blockIdx.x] = (x > y) ? L - 1 : END;
    }
}

/* decode.c:1513-1523, one thread per read: path[blk] in 0..L-1, -1 for START and END */
__global__ __launch_bounds__(64) void k_map_walk(const ShMapRead *__restrict__ rd, int n, const unsigned *__restrict__ tb,
                                                 const int *__restrict__ final_state, const long long *__restrict__ path_off,
                                                 int *__restrict__ path) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShMapRead r = rd[i];
    if (!r.ok || r.tb < 0 || path_off[i] < 0) return;
    const int L = r.seqlen, NB = r.nblock, W = sh_map_words(L);
    const unsigned *w = tb + r.tb, *we = w + (long long)NB * W;
    int *out = path + path_off[i];
    int st = final_state[i];
    out[NB - 1] = st >= L ? -1 : st;
    for (int blk = NB - 1; blk > 0; blk--) {
        int prev;
        if (st == L) prev = L;
        else if (st == L + 1) prev = ((we[blk >> 5] >> (blk & 31)) & 1u) ? L - 1 : L + 1;
        else {
            const int code = (int)((w[(long long)blk * W + (st >> 4)] >> (2 * (st & 15))) & 3u);
            prev = code == 3 ? L : st - code;
        }
        out[blk - 1] = prev >= L ? -1 : prev;
        st = prev;
    }
}

#endif /* SH_MAP_H */
