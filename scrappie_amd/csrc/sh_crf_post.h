/* sh_crf_post.h -- part of sh_kernels.h (included from there, behind sh_crf.h): the posterior over the five flip-flop states at every block boundary
 * (posterior_crf, decode.c:928-1012) as a forward / backward pass over a read's normalised transitions.
 * Device code for gfx950 only; see sh_kernels.h for conventions (layouts, citations). */
#ifndef SH_CRF_POST_H
#define SH_CRF_POST_H

/* Where the transitions of a tile's reads lie: the two loaders of k_crf_post.  A loader hands every lane a view of ITS read: col(t), the base of
 * block t's column clamped into what the read (or its tile) owns, and slot(e), where element e (< 32) of a column is from there.  Elements 25 .. 31
 * are what a lane without a state loads and throws away: padding where the layout has some, any of the read's own 25 where it has none. */

/* (a) the engine's tiled layout, where k_crf<true> leaves the normalised transitions: 512 floats per block and tile, element e of read b at
 * (e >> 4) * 256 + (((e >> 2) & 3) * 16 + b) * 4 + (e & 3) */
struct ShCrfTiled {
    const float *C;
    const long long *tile_boff;
    struct View {
        const float *base; int b, last;
        __device__ __forceinline__ const float *col(int t) const { return base + (long long)min(max(t, 0), last) * 512; }
        __device__ __forceinline__ int slot(int e) const { return (e >> 4) * 256 + (((e >> 2) & 3) * 16 + b) * 4 + (e & 3); }
    };
    __device__ __forceinline__ View view(int tile, int b, int, int, int Tt) const { return View{C + tile_boff[tile] * 512, b, Tt - 1}; }
};
/* (b) reference-layout matrices from the host (nr = 25, each with its own column stride), one per read, side by side: what decode_crf's batch reads */
struct ShCrfRef {
    const float *trans;
    const long long *foff;          /* [npad] first float of the read's matrix */
    const int *stride;              /* [npad] */
    struct View {
        const float *base; int stride, last;
        __device__ __forceinline__ const float *col(int t) const { return base + (long long)min(max(t, 0), last) * stride; }
        __device__ __forceinline__ int slot(int e) const { return min(e, 24); }
    };
    __device__ __forceinline__ View view(int, int, int rd, int T, int) const { return View{trans + foff[rd], stride[rd], T - 1}; }
};

/* One tile of 16 reads per 128-thread workgroup, 8 lanes per read, as k_crf (sh_crf.h).  Forward pass: lane s < 5 owns the transitions INTO state s
 * (elements 5 s .. 5 s + 4) and runs that state's chain over the source states 0 .. 4 in the reference's order (decode.c:951-957); the forward
 * messages of blocks 0 .. T go to the read's own output columns, as the reference keeps them in `post`.  Backward pass: lane s owns the transitions
 * OUT of state s (elements s, 5 + s, .., 20 + s: the transposed pick of the same 25 floats), chains over the target states 0 .. 4 (decode.c:987-995),
 * reads the forward message of its column back -- this same wave stored it earlier in program order, and a fence stands between the passes -- adds
 * the backward one, and the five lanes normalise: the column total starts at 0.0f and takes states 0 .. 4 in order (quirk Q16: every total carries
 * an extra e^0, so a column sums to less than one), and the probabilities overwrite the messages.  The last column is normalised from the forward
 * messages alone (decode.c:969-975).  The five messages cross lanes once per block and pass (__shfl inside the read's 8 lanes), the column total
 * once more in the backward pass.
 * As in k_crf, every vector-memory operation of the two block loops is UNCONDITIONAL, so that the compiler can count what is in flight (vmcnt) and
 * the ring of D columns runs ahead: loops run to the TILE's block count, every lane loads five floats it may read, what a lane has no use for is
 * dropped by a select, and the stores of lanes 5 - 7 and of blocks past the read's own end go to `dump` (one float per thread, never read).
 * Output: [T + 1][5] floats per read at out + ooff[rd] (the host's plan, scrappie_hip_crf_post_plan); nothing else of `out` is written. */
template <class L>
__global__ __launch_bounds__(128) void k_crf_post(L ld, const int *__restrict__ rT /*[npad]*/, const int *__restrict__ tile_T /*[ntile]*/,
                                                  const long long *__restrict__ ooff /*[npad]*/, float *out, float *dump /*[128]*/) {
    const int tile = blockIdx.x;
    const int b = threadIdx.x >> 3, st = threadIdx.x & 7;
    const int lane = threadIdx.x & 63, grp = lane & ~7;
    const int rd = tile * 16 + b;
    const int T = rT[rd];                          /* the 8 lanes of a read agree; the shuffles below stay inside them */
    const int Tt = tile_T[tile];                   /* (uniform) */
    if (T <= 0) return;
    const auto v = ld.view(tile, b, rd, T, Tt);
    const bool own = st < 5;
    const int sc = min(st, 4);
    float *po = out + ooff[rd];
    float *pd = dump + threadIdx.x;
    int ef[5], eb[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int pad = st == 5 ? 25 + k : 28 + ((st - 6) * 5 + k) % 4;          /* <= 31 */
        ef[k] = v.slot(own ? 5 * st + k : pad);
        eb[k] = v.slot(own ? 5 * k + st : pad);
    }
    auto gather = [&](float mine, float (&p)[5]) {
#pragma unroll
        for (int k = 0; k < 5; k++) p[k] = __shfl(mine, grp + k);
    };
    /* the column total of five values held by lanes grp .. grp + 4, Q16 and all, and mine over it.  The argument of the exponential is <= 0 by
     * construction but not bounded below (a state no path reaches: -1e4 and less), so it is d_exp with its clamp, not the raw exponential. */
    auto normalise = [&](float mine) {
        float p[5];
        gather(mine, p);
        float tot = 0.0f;
#pragma unroll
        for (int s = 0; s < 5; s++) tot = d_lse(tot, p[s]);
        return d_exp(mine - tot);
    };
    constexpr int D = SH_CRF_D;
    float q[D][5];
    /* The ring's first D columns are waited for in full before a block loop is entered (s_waitcnt vmcnt(0), expcnt and lgkmcnt left alone: one round
     * trip per pass).  The compiler orders those D x 5 loads as it likes, and the one count it may put in front of the loop's first use has to hold on
     * both ways in, from here and round the loop: with loads of the first column among the last issued here it came out as "everything but this
     * block's own loads", on every trip, and the ring ran one block ahead instead of D. */
    auto ring_primed = [] { __builtin_amdgcn_s_waitcnt(0x0f70); };
    /* For the same reason a block fetches column t +- D into q[d] BEHIND its own store, after its last use of q[d]: the store may alias the loads as
     * far as the compiler knows, so they stay there, the new column lands in the registers the old one has left, and the loop needs no copies at
     * its end.  (Fetched before the use, old and new column were live together, every trip ended with D x 5 register moves, and those wait for
     * every load in flight.) */

    /* forward */
    auto fetch_f = [&](int t, float (&x)[5]) {
        const float *col = v.col(t);
#pragma unroll
        for (int k = 0; k < 5; k++) x[k] = col[ef[k]];
    };
    float mine = 0.0f;
    *(own ? po + st : pd) = 0.0f;                  /* column 0 (decode.c:940-943) */
#pragma unroll
    for (int d = 0; d < D; d++) fetch_f(d, q[d]);
    ring_primed();
    for (int t0 = 0; t0 < Tt; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const int t = t0 + d;
            float p[5];
            gather(mine, p);
            float acc = q[d][0] + p[0];
#pragma unroll
            for (int fr = 1; fr < 5; fr++) acc = d_lse(acc, q[d][fr] + p[fr]);
            const bool live = t < T;
            mine = live ? acc : mine;
            *((live && own) ? po + (long long)(t + 1) * 5 + st : pd) = mine;
            fetch_f(t + D, q[d]);          /* behind the block's last use of q[d]: the same registers take the new column, see above */
        }
    }
    /* the last column from the forward messages alone */
    *(own ? po + (long long)T * 5 + st : pd) = normalise(mine);
    __threadfence();                               /* the forward messages are read back below */

    /* backward: blocks Tt - 1 .. 0; a read shorter than its tile waits with a zero message until its own last block */
    float a[D];
    auto fetch_b = [&](int t, float (&x)[5], float &al) {
        const float *col = v.col(t);
#pragma unroll
        for (int k = 0; k < 5; k++) x[k] = col[eb[k]];
        al = po[(long long)min(max(t, 0), T - 1) * 5 + sc];       /* (column t is overwritten in iteration t, behind this load; lanes 5 - 7 and t >= T: dropped) */
    };
    mine = 0.0f;
#pragma unroll
    for (int d = 0; d < D; d++) fetch_b(Tt - 1 - d, q[d], a[d]);
    ring_primed();
    for (int t0 = Tt - 1; t0 >= 0; t0 -= D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const int t = t0 - d;
            float p[5];
            gather(mine, p);
            float acc = q[d][0] + p[0];
#pragma unroll
            for (int to = 1; to < 5; to++) acc = d_lse(acc, q[d][to] + p[to]);
            const bool live = t >= 0 && t < T;
            mine = live ? acc : mine;
            const float pr = normalise(a[d] + mine);
            *((live && own) ? po + (long long)t * 5 + st : pd) = pr;
            fetch_b(t - D, q[d], a[d]);
        }
    }
}

#endif /* SH_CRF_POST_H */
