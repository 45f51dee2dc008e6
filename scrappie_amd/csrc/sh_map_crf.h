/* sh_map_crf.h -- part of sh_kernels.h (included from there, behind sh_crf_post.h): a read of a flip-flop (CRF) model mapped to a
 * base sequence, block by block.  decode_crf's recursion (decode.c:836-893) restricted to the paths that spell the sequence:
 * the Viterbi score, its path, and the forward score, full or inside a band.  The reference has no such function; the
 * definition is decode_crf's own, and mapping a read to its own call returns decode_crf's score bit for bit.
 *
 * A read's transitions: 25 floats per block, element to * 5 + from, states A C G T stay (4).  A path has nblock + 1 entries;
 * its non-stay entries, in order, are exactly seq[0..L).  After an entry the path is in cell (p, kind), p = 0..L the bases
 * emitted so far: B[p] (p >= 1) where the entry was base seq[p - 1], S[p] where it was a stay.  Entry 0: B[1] = S[0] = 0,
 * everything else -SH_MAP_BIG.  Block t, with b = seq[p - 1], in float32 as tr + prev, the base predecessor first, then stay,
 * replaced on strict > (decode_crf's order: from-state ascending, stay last):
 *     B'[p] = max(tr[5 b + seq[p - 2]] + B[p - 1]   (p >= 2),   tr[5 b + 4] + S[p - 1])
 *     S'[p] = max(tr[20 + b] + B[p]                 (p >= 1),   tr[24] + S[p])
 * End: B[L] if B[L] >= S[L], else S[L].  Forward: sh_lse in place of max, the terms in the same order.  The build has
 * -ffp-contract=off, and the Viterbi form holds additions and compares only.
 *
 * Band: cell index p of entry t lies in [low[t], high[t]) (nblock + 1 entries each; the host has checked them:
 * scrappie_hip_map_crf_bounds_sane).  Once the row of entry t is complete, every cell outside its band holds -SH_MAP_BIG, as in
 * k_squig_band: a read of the previous row is predicated on the previous entry's band, with the constant outside; nothing is
 * ever cleared, and only the band's cells are computed, so a read costs entries x width.  A read without a band has the full
 * band [0, L + 1) at every entry and runs through the same code: a band that contains the unbanded Viterbi path gives the
 * unbanded score and path bit for bit (the first maximum stays the first when other candidates only become smaller).
 *
 * Work split, as k_map: one workgroup of SH_MAP_NTH threads per read; the cells of an entry are independent given the previous
 * entry's row, cell p on thread p % SH_MAP_NTH (from the 64-cell group that holds low[t] on, inside a band).  Two ping-pong
 * buffers, each a B row and an S row of L + 2 floats (cells 0 .. L, then a slot that takes the stores of threads without a
 * cell); one barrier per block.  Rows and base codes live in LDS while SH_MAPC_HEAD + 4 (L + 2) + L words fit SH_MAP_LDS, the
 * rows in device scratch beyond (the codes are then read from the read's own array): two instantiations, a launch holds reads
 * of one home, and a pointer never selects between LDS and global memory at run time.
 * Transitions: through the loaders' views of sh_crf_post.h (ShCrfTiled::View on what k_crf<true> left in d_E, ShCrfRef::View on
 * a host matrix): thread e & 31 loads element slot(e) of a column, SH_MAPC_D columns ahead of the block that uses it, and hands
 * it over through two 32-float LDS columns.  Every vector-memory operation of the block loop but the traceback store is
 * unconditional -- columns past the read's end clamp (col), indices clamp and a select drops the value, stores without a
 * cell go to the spare slot -- so the compiler can count what is in flight and the columns run ahead.  (A banded read also
 * loads the next entry's two edges per block, behind a branch the whole workgroup takes alike.)
 *
 * Traceback (Viterbi, where a path is wanted): one bit per cell and kind -- 1: the predecessor was the stay cell -- per block:
 * two wave-ballot planes per 64 cells, {B low, B high, S low, S high} as one 16-byte store by the wave's first lane;
 * W = 4 ceil((L + 1) / 64) words per block, indexed by the cell, not by the band.  The end's kind per read in final_state
 * (0: B, 1: S, -1: no admissible path -- a score below -SH_MAP_BIG / 2; the host answers NAN).  k_map_crf_walk, one thread per
 * read: path[t] = index of the last base emitted through entry t, -1 while none.  A finite path never enters a masked cell,
 * so the walk reads only words the kernel wrote.  All stores are plain vector stores.
 */
#ifndef SH_MAP_CRF_H
#define SH_MAP_CRF_H

#include "sh_map.h"     /* SH_MAP_NTH, SH_MAP_LDS, SH_MAP_MAX_SEQ, SH_MAP_BIG, sh_lse */

#define SH_MAPC_D 4               /* transition columns in flight per workgroup */
#define SH_MAPC_HEAD 64           /* LDS floats in front of the rows: two columns of 32 (25 used) */

struct ShMapCrfRead {
    long long trans;    /* tiled: the first column block of the read's tile; reference layout: float offset of the read's matrix */
    long long tb;       /* first traceback word (multiple of 4); -1: no traceback */
    long long scr;      /* float offset of the four score rows in device scratch; -1: in LDS */
    long long seq;      /* offset of the read's base codes */
    long long band;     /* offset of low (nblock + 1 int32) and high (the next nblock + 1); -1: the full band */
    int nblock, seqlen;
    int lane;           /* tiled: the read's lane in its tile (0..15); reference layout: the matrix's column stride */
    int ok;             /* 0: nothing to do (the host has set NAN) */
};

struct ShMapCrfArgs {
    const ShMapCrfRead *rd;
    const float *trans;         /* d_E, or the uploaded matrices */
    const int *seq;
    const int *band;
    unsigned *tb;
    float *scr;
    float *score;               /* [read] */
    int *final_state;           /* [read] Viterbi: 0 the path ends in B[L], 1 in S[L], -1 none */
};

__device__ __forceinline__ int sh_map_crf_words(int L) { return 4 * ((L + 64) / 64); }

template <class LOADER> struct ShMapCrfView;
template <> struct ShMapCrfView<ShCrfTiled> {
    static __device__ __forceinline__ ShCrfTiled::View make(const float *tr, const ShMapCrfRead &r) { return ShCrfTiled::View{tr + r.trans * 512, r.lane, r.nblock - 1}; }
};
template <> struct ShMapCrfView<ShCrfRef> {
    static __device__ __forceinline__ ShCrfRef::View make(const float *tr, const ShMapCrfRead &r) { return ShCrfRef::View{tr + r.trans, r.lane, r.nblock - 1}; }
};

/* One cell of block t, for k_map_crf and k_map_crf_pack (sh_map_crf_pack.h) alike: tr the block's column, tSS = tr[24], b = seq[p - 1] and
 * bp = seq[p - 2] (any base where there is none), p the cell (k_map_crf_pack: 0, 1 or 2 for p >= 2), (B0, S0) the previous entry's cell p and
 * (B1, S1) its cell p - 1, -SH_MAP_BIG where there is none.  vb, vs: B'[p] and S'[p]; kb, ks (Viterbi): the predecessor was the stay cell. */
template <bool VIT>
__device__ __forceinline__ void sh_map_crf_cell(const float *tr, float tSS, int b, int bp, int p, float B0, float S0, float B1, float S1,
                                                float &vb, float &vs, bool &kb, bool &ks) {
    const float bb = tr[5 * b + bp] + B1, bs = tr[5 * b + 4] + S1;
    const float sb = tr[20 + b] + B0, ss = tSS + S0;
    if (VIT) {
        kb = p < 2 || bs > bb; vb = kb ? bs : bb;
        ks = p < 1 || ss > sb; vs = ks ? ss : sb;
    } else {
        kb = ks = false;
        vb = p < 2 ? bs : sh_lse(bb, bs);
        vs = p < 1 ? ss : sh_lse(sb, ss);
    }
    if (p < 1) vb = -SH_MAP_BIG;                             /* there is no B[0] */
}

template <bool VIT, class LOADER, bool LDS>
__global__ __launch_bounds__(SH_MAP_NTH) void k_map_crf(ShMapCrfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_mapc_lds[];
    const ShMapCrfRead r = a.rd[blockIdx.x];
    if (!r.ok) return;
    const int tid = threadIdx.x, L = r.seqlen, NB = r.nblock, RW = L + 2, SPARE = L + 1;
    float *const trb = sh_mapc_lds;                          /* [2][32] */
    float *const buf0 = LDS ? sh_mapc_lds + SH_MAPC_HEAD : a.scr + r.scr;
    float *const buf1 = buf0 + 2 * RW;
    int *const lds_seq = (int *)(sh_mapc_lds + SH_MAPC_HEAD + 4 * RW);
    if (LDS)
        for (int i = tid; i < L; i += SH_MAP_NTH) lds_seq[i] = a.seq[r.seq + i];
    const int *const sq = LDS ? (const int *)lds_seq : a.seq + r.seq;
    const bool banded = r.band >= 0;                         /* (uniform) */
    const int *const blo = a.band + (banded ? r.band : 0), *const bhi = blo + (NB + 1);
    int lo_p = 0, hi_p = banded ? bhi[0] : L + 1;            /* the band of the previous entry's row */
    int lo_c = banded ? blo[1] : 0, hi_c = banded ? bhi[1] : L + 1;
    for (int p = tid; p < hi_p; p += SH_MAP_NTH) {           /* entry 0, its band's cells only */
        buf0[p] = p == 1 ? 0.0f : -SH_MAP_BIG;
        buf0[RW + p] = p == 0 ? 0.0f : -SH_MAP_BIG;
    }
    const auto v = ShMapCrfView<LOADER>::make(a.trans, r);
    const int slot = v.slot(tid & 31);
    float q[SH_MAPC_D];                                      /* q[d]: the column of block t0 + d + 1 */
    if (tid < 32) trb[tid] = v.col(0)[slot];
#pragma unroll
    for (int d = 0; d < SH_MAPC_D; d++) q[d] = v.col(d + 1)[slot];
    const bool want_tb = VIT && r.tb >= 0;
    const int W = sh_map_crf_words(L);
    unsigned *const tbw = want_tb ? a.tb + r.tb : nullptr;
    const int wv = tid >> 6;
    __syncthreads();
    for (int t0 = 0; t0 < NB; t0 += SH_MAPC_D) {
#pragma unroll
        for (int d = 0; d < SH_MAPC_D; d++) {
            const int t = t0 + d;                            /* block t: entry t -> entry t + 1 */
            if (t >= NB) break;                              /* (uniform) */
            const float *const pB = (t & 1) ? buf1 : buf0, *const pS = pB + RW;
            float *const cB = (t & 1) ? buf0 : buf1, *const cS = cB + RW;
            const float *const tr = trb + (t & 1) * 32;
            const int nx = min(t + 2, NB);
            const int lo_n = banded ? blo[nx] : 0, hi_n = banded ? bhi[nx] : L + 1;      /* asked for before the barrier */
            const float tSS = tr[24];
            const int base = lo_c & ~63;
            const int nch = (hi_c - base + SH_MAP_NTH - 1) / SH_MAP_NTH;
            for (int ch = 0; ch < nch; ch++) {
                const int p = base + ch * SH_MAP_NTH + tid;
                const bool valid = p >= lo_c && p < hi_c;
                const int p0 = min(p, L), p1 = min(max(p - 1, 0), L);
                const int b = sq[min(max(p - 1, 0), L - 1)], bp = sq[min(max(p - 2, 0), L - 1)];
                const bool in0 = p >= lo_p && p < hi_p, in1 = p - 1 >= lo_p && p - 1 < hi_p;
                const float lB0 = pB[p0], lS0 = pS[p0], lB1 = pB[p1], lS1 = pS[p1];
                const float B0 = in0 ? lB0 : -SH_MAP_BIG, S0 = in0 ? lS0 : -SH_MAP_BIG;
                const float B1 = in1 ? lB1 : -SH_MAP_BIG, S1 = in1 ? lS1 : -SH_MAP_BIG;
                float vb, vs;
                bool kb, ks;
                sh_map_crf_cell<VIT>(tr, tSS, b, bp, p, B0, S0, B1, S1, vb, vs, kb, ks);
                const int at = valid ? p : SPARE;
                cB[at] = vb;
                cS[at] = vs;
                if (want_tb) {
                    const unsigned long long m0 = __ballot(valid && kb), m1 = __ballot(valid && ks), any = __ballot(valid);
                    if ((tid & 63) == 0 && any != 0ull) {    /* a group with a valid cell: (base >> 6) + 4 ch + wv <= L >> 6 < W / 4 */
                        const int g = (base >> 6) + ch * (SH_MAP_NTH / 64) + wv;
                        *(uint4 *)(tbw + (long long)t * W + (long long)g * 4) =
                            make_uint4((unsigned)m0, (unsigned)(m0 >> 32), (unsigned)m1, (unsigned)(m1 >> 32));
                    }
                }
            }
            if (tid < 32) trb[((t + 1) & 1) * 32 + tid] = q[d];     /* block t + 1's column; read last in block t - 1, a barrier ago */
            q[d] = v.col(t + 1 + SH_MAPC_D)[slot];
            lo_p = lo_c; hi_p = hi_c; lo_c = lo_n; hi_c = hi_n;
            __syncthreads();
        }
    }
    if (tid == 0) {                                          /* entry NB: its band holds cell L (high[NB] = L + 1) */
        const float *const f = (NB & 1) ? buf1 : buf0;
        const float x = f[L], y = f[RW + L];
        const float sc = VIT ? (x >= y ? x : y) : sh_lse(x, y);
        a.score[blockIdx.x] = sc;
        if (VIT && a.final_state) a.final_state[blockIdx.x] = sc < -SH_MAP_BIG / 2 ? -1 : (x >= y ? 0 : 1);
    }
}

/* one thread per read: path[t], t = 0 .. nblock, from the end's kind and the predecessor bits */
__global__ __launch_bounds__(64) void k_map_crf_walk(const ShMapCrfRead *__restrict__ rd, int n, const unsigned *__restrict__ tb,
                                                     const int *__restrict__ final_state, const long long *__restrict__ path_off,
                                                     int *__restrict__ path) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShMapCrfRead r = rd[i];
    if (!r.ok || r.tb < 0 || path_off[i] < 0) return;
    int kind = final_state[i];
    if (kind < 0) return;                            /* no path */
    const int L = r.seqlen, NB = r.nblock, W = sh_map_crf_words(L);
    const unsigned *w = tb + r.tb;
    int *out = path + path_off[i];
    int p = L;
    for (int t = NB; t >= 1; t--) {
        out[t] = p - 1;
        const unsigned word = w[(long long)(t - 1) * W + (long long)(p >> 6) * 4 + (kind ? 2 : 0) + ((p & 63) >> 5)];
        const int stay = (int)((word >> (p & 31)) & 1u);
        if (kind == 0 && p > 0) p--;                 /* (a finite path never has p = 0 here; never index below the codes) */
        kind = stay;
    }
    out[0] = p - 1;
}

#endif /* SH_MAP_CRF_H */
