/* sh_map_crf_local.h -- part of sh_kernels.h (included from there, behind sh_map_crf.h): a read of a flip-flop (CRF) model mapped INTO a
 * longer base sequence: where in the sequence the read lies, with what score and along what path.  The reference has no such
 * function; as for k_map_crf the definition is decode_crf's own recursion (decode.c:836-893), restricted to the paths that spell a
 * stretch seq[first, last) of the sequence.  Mapping a read to flank + its own call + flank returns decode_crf's score bit for bit.
 *
 * Cells, transitions and the block recursion are sh_map_crf.h's: cells (p, kind), p = 0 .. L the bases of the sequence behind the
 * path, B[p] (the entry was base seq[p - 1]) and S[p] (a stay); float32 as tr + prev, the base predecessor first, then stay,
 * replaced on strict >; -ffp-contract=off.  Two things differ.
 *   Entry 0: the path may begin anywhere: S[p] = 0 for p = 0 .. L, B[p] = 0 for p = 1 .. L (decode_crf starts every state at 0).
 *   End: the path may end anywhere: Viterbi the maximum over all cells of entry nblock, scanned with p ascending and B[p] before
 *   S[p], the first maximum wins; forward sh_lse over the same cells.  The read spells seq[first, last): last the end cell's p,
 *   first the start cell's p, minus one where entry 0 is a base.  path[t] = p_t - 1, the index in seq of the last base emitted
 *   through entry t, first - 1 while there is none.  The all-stay path is always admissible: there is no "no path" here.
 *
 * Windows.  The cells of an entry are independent and a path advances at most one cell per block, so the sequence is cut into
 * windows that never talk to each other, one workgroup of SH_MAP_NTH threads each.  Window w of stride s OWNS the paths whose start
 * cell lies in [w s, min((w + 1) s, L + 1)): only those cells are 0 at entry 0, all others -SH_MAP_BIG.  Its cells are
 * [w s, min(w s + s - 1 + nblock, L)]; a cell to the left of the window is never a predecessor of an owned path, and reads as
 * -SH_MAP_BIG.  Every path is owned by exactly one window and lies wholly inside it, and a path's score is the same chain of float
 * additions wherever it is computed: the Viterbi score is bit-identical for every stride, one window included.  The host takes the
 * highest window (the lowest on a tie), or sh_lse over the windows in their order (ownership is a partition: nothing counts twice).
 * The cut itself is host arithmetic: scrappie_hip_map_crf_local_plan (sh_host.c).
 *
 * Inside a window everything is k_map_crf's: cell c0 + j on thread j % SH_MAP_NTH, two ping-pong buffers of a B row and an S row
 * of ncell + 1 floats (the window's cells, then a slot that takes the stores of threads without a cell), one barrier per block;
 * rows and codes in LDS while SH_MAPC_HEAD + 4 (ncell + 1) + ncell words fit SH_MAP_LDS, the rows in device scratch beyond (the
 * codes are then read from the sequence itself): two instantiations, never a pointer that chooses at run time.  Transitions through
 * the ShCrfTiled::View / ShCrfRef::View column ring, SH_MAPC_D columns ahead; every vector-memory operation of the block loop but
 * the traceback store is unconditional.
 *
 * End of a window: every thread scans its cells in order (j ascending, B before S), then six __shfl_xor steps inside the wave,
 * then the four waves through LDS, thread 0 last.  Viterbi carries (score, 2 j + kind): the higher score, on equal scores the
 * lower key -- the first maximum of the scan whatever the order of the reduction.  Forward: acc = -SH_MAP_BIG, then
 * acc = sh_lse(acc, x) per cell (sh_lse(-SH_MAP_BIG, x) is x), sh_lse(acc, __shfl_xor(acc, d)) for d = 1, 2 .. 32 (sh_lse is
 * symmetric: every lane of a wave ends with the same bits), then wave 0 .. 3 in order.  One score per window; Viterbi also the end
 * cell (its p in the sequence) and kind.
 *
 * Traceback (the second pass, on a read's best window alone): k_map_crf's layout -- one bit per cell and kind per block, two
 * wave-ballot planes per 64 cells as one 16-byte store -- indexed by the cell IN the window, W = 4 ceil(ncell / 64) words per
 * block.  k_map_crf_local_walk, one thread per window: path[t] and first.  All stores are plain vector stores. */
#ifndef SH_MAP_CRF_LOCAL_H
#define SH_MAP_CRF_LOCAL_H

#include "sh_map_crf.h"

struct ShMapCrfLocalWin {
    long long trans;    /* tiled: the first column block of the read's tile; reference layout: float offset of the read's matrix */
    long long tb;       /* first traceback word (multiple of 4); -1: no traceback */
    long long scr;      /* float offset of the four score rows in device scratch; -1: in LDS */
    long long seq;      /* offset of the sequence's code 0 */
    int nblock, seqlen;
    int lane;           /* tiled: the read's lane in its tile (0..15); reference layout: the matrix's column stride */
    int first;          /* the window's first cell */
    int ncell;          /* its cells: first .. first + ncell - 1 <= seqlen */
    int own;            /* the start cells it owns: first .. first + own - 1 */
    int ok;             /* 0: nothing to do */
    int pad_;
};

struct ShMapCrfLocalArgs {
    const ShMapCrfLocalWin *rd;
    const float *trans;         /* d_E, or the uploaded matrices */
    const int *seq;
    unsigned *tb;
    float *scr;
    float *score;               /* [window] */
    int2 *final_state;          /* [window] Viterbi: (the end cell's p, its kind: 0 B, 1 S) */
};

__device__ __forceinline__ int sh_map_crf_local_words(int ncell) { return 4 * ((ncell + 63) / 64); }

template <class LOADER> struct ShMapCrfLocalView;
template <> struct ShMapCrfLocalView<ShCrfTiled> {
    static __device__ __forceinline__ ShCrfTiled::View make(const float *tr, const ShMapCrfLocalWin &r) { return ShCrfTiled::View{tr + r.trans * 512, r.lane, r.nblock - 1}; }
};
template <> struct ShMapCrfLocalView<ShCrfRef> {
    static __device__ __forceinline__ ShCrfRef::View make(const float *tr, const ShMapCrfLocalWin &r) { return ShCrfRef::View{tr + r.trans, r.lane, r.nblock - 1}; }
};

template <bool VIT, class LOADER, bool LDS>
__global__ __launch_bounds__(SH_MAP_NTH) void k_map_crf_local(ShMapCrfLocalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sh_mapl_lds[];
    const ShMapCrfLocalWin r = a.rd[blockIdx.x];
    if (!r.ok) return;
    const int tid = threadIdx.x, L = r.seqlen, NB = r.nblock, NC = r.ncell, c0 = r.first, RW = NC + 1, SPARE = NC;
    float *const trb = sh_mapl_lds;                          /* [2][32]; after the block loop: the waves' results */
    float *const buf0 = LDS ? sh_mapl_lds + SH_MAPC_HEAD : a.scr + r.scr;
    float *const buf1 = buf0 + 2 * RW;
    int *const lds_seq = (int *)(sh_mapl_lds + SH_MAPC_HEAD + 4 * RW);      /* [j]: seq[c0 + j - 1], the base of cell j */
    const int *const gseq = a.seq + r.seq;
    if (LDS)
        for (int j = tid; j < NC; j += SH_MAP_NTH) lds_seq[j] = gseq[min(max(c0 + j - 1, 0), L - 1)];
    for (int j = tid; j < NC; j += SH_MAP_NTH) {             /* entry 0: the start cells this window owns */
        const bool mine = j < r.own;
        buf0[j] = mine && c0 + j >= 1 ? 0.0f : -SH_MAP_BIG;
        buf0[RW + j] = mine ? 0.0f : -SH_MAP_BIG;
    }
    const auto v = ShMapCrfLocalView<LOADER>::make(a.trans, r);
    const int slot = v.slot(tid & 31);
    float q[SH_MAPC_D];                                      /* q[d]: the column of block t0 + d + 1 */
    if (tid < 32) trb[tid] = v.col(0)[slot];
#pragma unroll
    for (int d = 0; d < SH_MAPC_D; d++) q[d] = v.col(d + 1)[slot];
    const bool want_tb = VIT && r.tb >= 0;
    const int W = sh_map_crf_local_words(NC);
    unsigned *const tbw = want_tb ? a.tb + r.tb : nullptr;
    const int wv = tid >> 6;
    const int nch = (NC + SH_MAP_NTH - 1) / SH_MAP_NTH;
    __syncthreads();
    for (int t0 = 0; t0 < NB; t0 += SH_MAPC_D) {
#pragma unroll
        for (int d = 0; d < SH_MAPC_D; d++) {
            const int t = t0 + d;                            /* block t: entry t -> entry t + 1 */
            if (t >= NB) break;                              /* (uniform) */
            const float *const pB = (t & 1) ? buf1 : buf0, *const pS = pB + RW;
            float *const cB = (t & 1) ? buf0 : buf1, *const cS = cB + RW;
            const float *const tr = trb + (t & 1) * 32;
            const float tSS = tr[24];
            for (int ch = 0; ch < nch; ch++) {
                const int j = ch * SH_MAP_NTH + tid, p = c0 + j;
                const bool valid = j < NC;
                const int j0 = min(j, NC - 1), j1 = min(max(j - 1, 0), NC - 1);
                int b, bp;
                if (LDS) { b = lds_seq[j0]; bp = lds_seq[j1]; }
                else { b = gseq[min(max(p - 1, 0), L - 1)]; bp = gseq[min(max(p - 2, 0), L - 1)]; }
                const float B0 = pB[j0], S0 = pS[j0], lB1 = pB[j1], lS1 = pS[j1];
                const float B1 = j >= 1 ? lB1 : -SH_MAP_BIG, S1 = j >= 1 ? lS1 : -SH_MAP_BIG;    /* left of the window: no owned path */
                const float bb = tr[5 * b + bp] + B1, bs = tr[5 * b + 4] + S1;
                const float sb = tr[20 + b] + B0, ss = tSS + S0;
                float vb, vs;
                bool kb, ks;
                if (VIT) {
                    kb = p < 2 || bs > bb; vb = kb ? bs : bb;
                    ks = p < 1 || ss > sb; vs = ks ? ss : sb;
                } else {
                    kb = ks = false;
                    vb = p < 2 ? bs : sh_lse(bb, bs);
                    vs = p < 1 ? ss : sh_lse(sb, ss);
                }
                if (p < 1) vb = -SH_MAP_BIG;                 /* there is no B[0] */
                const int at = valid ? j : SPARE;
                cB[at] = vb;
                cS[at] = vs;
                if (want_tb) {
                    const unsigned long long m0 = __ballot(valid && kb), m1 = __ballot(valid && ks), any = __ballot(valid);
                    if ((tid & 63) == 0 && any != 0ull) {    /* a group with a valid cell: 4 ch + wv <= (NC - 1) >> 6 < W / 4 */
                        const int g = ch * (SH_MAP_NTH / 64) + wv;
                        *(uint4 *)(tbw + (long long)t * W + (long long)g * 4) =
                            make_uint4((unsigned)m0, (unsigned)(m0 >> 32), (unsigned)m1, (unsigned)(m1 >> 32));
                    }
                }
            }
            if (tid < 32) trb[((t + 1) & 1) * 32 + tid] = q[d];     /* block t + 1's column; read last in block t - 1, a barrier ago */
            q[d] = v.col(t + 1 + SH_MAPC_D)[slot];
            __syncthreads();
        }
    }
    /* entry NB: the window's end.  (trb is free: the last column was read before the loop's last barrier) */
    const float *const fB = (NB & 1) ? buf1 : buf0, *const fS = fB + RW;
    float acc = -SH_MAP_BIG;
    int key = 0x7fffffff;                                    /* 2 j + kind */
    for (int j = tid; j < NC; j += SH_MAP_NTH) {
        const float x = fB[j], y = fS[j];
        if (VIT) {
            if (x > acc || key == 0x7fffffff) { acc = x; key = 2 * j; }
            if (y > acc) { acc = y; key = 2 * j + 1; }
        } else {
            acc = sh_lse(acc, x);
            acc = sh_lse(acc, y);
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float ov = __shfl_xor(acc, d);
        if (VIT) {
            const int ok = __shfl_xor(key, d);
            if (ov > acc || (ov == acc && ok < key)) { acc = ov; key = ok; }
        } else {
            acc = sh_lse(acc, ov);
        }
    }
    if ((tid & 63) == 0) { trb[wv] = acc; ((int *)trb)[8 + wv] = key; }
    __syncthreads();
    if (tid == 0) {
        float sc = trb[0];
        int k = ((const int *)trb)[8];
        for (int w = 1; w < SH_MAP_NTH / 64; w++) {
            const float ov = trb[w];
            const int ok = ((const int *)trb)[8 + w];
            if (VIT) { if (ov > sc || (ov == sc && ok < k)) { sc = ov; k = ok; } }
            else sc = sh_lse(sc, ov);
        }
        a.score[blockIdx.x] = sc;
        if (VIT && a.final_state) a.final_state[blockIdx.x] = make_int2(c0 + (k >> 1), k & 1);
    }
}

/* one thread per window: path[t] = p_t - 1, t = 0 .. nblock, from the end cell and the predecessor bits; first[i] = the start
 * cell's p, minus one where entry 0 is a base */
__global__ __launch_bounds__(64) void k_map_crf_local_walk(const ShMapCrfLocalWin *__restrict__ rd, int n, const unsigned *__restrict__ tb,
                                                           const int2 *__restrict__ final_state, const long long *__restrict__ path_off,
                                                           int *__restrict__ path, int *__restrict__ first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShMapCrfLocalWin r = rd[i];
    if (!r.ok || r.tb < 0 || path_off[i] < 0) return;
    const int2 fs = final_state[i];
    const int NB = r.nblock, NC = r.ncell, c0 = r.first, W = sh_map_crf_local_words(NC);
    const unsigned *w = tb + r.tb;
    int *out = path + path_off[i];
    int j = min(max(fs.x - c0, 0), NC - 1), kind = fs.y;
    for (int t = NB; t >= 1; t--) {
        out[t] = c0 + j - 1;
        const unsigned word = w[(long long)(t - 1) * W + (long long)(j >> 6) * 4 + (kind ? 2 : 0) + ((j & 63) >> 5)];
        const int stay = (int)((word >> (j & 31)) & 1u);
        if (kind == 0 && j > 0) j--;                 /* (a path never leaves its window; never index below it) */
        kind = stay;
    }
    out[0] = c0 + j - 1;
    first[i] = c0 + j - (kind == 0 ? 1 : 0);
}

#endif /* SH_MAP_CRF_LOCAL_H */
