/* sh_dwell.h -- part of sh_kernels.h (included from there, behind sh_stitch.h): the dwell correction of homopolymer lengths, the last
 * step of `scrappie events` (decode.c:511-702), on the device: one lane per read, in the form of stitch_read / k_walk_stitch_out and for
 * their reason (sh_stitch.h): on host threads the step costs more than the device step it follows, and it wants the path (4 B per
 * event) on the host where the bases would do.  Kernels of their own: k_stitch and k_walk_stitch_out are not touched.
 *
 * Per read two sweeps over the path.  Sweep one: the length of the plain call (overlapper over every entry), and over the events the
 * sum of the dwells of the steps outside homopolymers and their number -- integers, so their order does not matter -- from which
 *     homo_scale = (float)((double)(prior_num / (float)plain_len + (float)tot_step_dwell) / (1.0 + nstep))
 * with every operation the reference's: a float division, a float addition, a double division rounded to float once.  Sweep two: the
 * corrected bases (and overlapper's pos[] when asked), a homopolymer of hdwell samples getting (int)roundf((float)hdwell / homo_scale)
 * bases: a float division and a round half away from zero.  All of these are exactly rounded IEEE operations here as on the host
 * (__fdiv_rn, __fadd_rn, __ddiv_rn: never the fast division), so the call is the host statement's (sh_host.c) bit for bit and no read
 * is left to the host for its arithmetic.
 *
 * The corrected length is known only behind the scale, so sweep two counts what it emits against the read's reservation and stores
 * nothing past it: a read that does not fit (a long dwell over a small scale), or whose count is no int, is flagged in redo[] and
 * stitched again by the host statement from the path still on the device.  What such a read had emitted before it ran out stays
 * behind in its own reservation (and its pos[] may be half written): nobody reads either, blen is 0 and the host writes both anew.
 *
 * Entries and events: the engine's path of a read of T events has T + 1 entries, and its plain call (and pos[]) is over all of them, as
 * for every other model; `scrappie events` pairs event ev with entry ev and stitches T entries (scrappie_events.c:300-316).  So the
 * correction walks the first nd = T entries, dwell[k] with entry k, and `ntrail` = 1 entry behind them counts for the plain length
 * alone.  (A read whose only k-mer is that last entry has no correction -- the reference is undefined there -- and keeps its plain
 * call.)  The test hook runs with ntrail = 0: path and events of the same length, as the reference's functions take them. */
#ifndef SH_DWELL_H
#define SH_DWELL_H

struct ShDwellArgs {
    const int *dwell;             /* (int)event.length of every event, read i at dwell_off[i] */
    const long long *dwell_off;   /* [npad] */
    const float *prior_num;       /* [npad] last.length + (float)(last.start - first.start) (decode.c:689-692) */
    const int *nd;                /* [npad] events of the read (<= 0: none) */
    const int *cap;               /* [npad] bytes the read owns at bases_off[i] (a multiple of 16) */
    int ntrail;                   /* path entries behind the last event: 1 in the engine, 0 in the test hook */
};

/* (returns what it leaves in blen[rd]; 0 with redo[rd] = 1: the host stitches this read) */
__device__ __forceinline__ int dwell_read(const ShStitchArgs &a, const ShDwellArgs &d, int rd) {
    const int nd = d.nd[rd];
    if (nd <= 0) { a.blen[rd] = -1; a.redo[rd] = 0; return -1; }
    const int n = nd + d.ntrail;
    const int *seq = a.seq + a.seq_off[rd];
    const int *dw = d.dwell + d.dwell_off[rd];
    const long long ss = a.sstride;
#define SQ(x) seq[(long long)(x) * ss]
#define PS(x) pos[(long long)(x) * ss]
    const int nkmer = a.nstate - 1;
    int klen = 0;
    for (int x = nkmer; x > 1; x >>= 2) klen++;

    /* sweep one: plain length; the scale's two sums over the events (decode.c:666-686 with pos[ev] as overlapper leaves it -- zero up to
     * and including the first k-mer -- and state[ev] = 1 + path[ev]) */
    int prev = -1, pp = 0, plain = 0;
    bool corr = false;                             /* a k-mer among the events: there is a correction */
    int tot = 0, nstep = 0, ppos = -2, evdwell = 0, pstate = -1;
    for (int k0 = 0; k0 < n; k0 += 8) {
        int v[8], w[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { v[u] = SQ(min(k0 + u, n - 1)); w[u] = dw[min(k0 + u, nd - 1)]; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int k = k0 + u, cur = v[u];
            if (k >= n) break;
            if (cur >= 0) {
                if (prev < 0) { plain = klen; corr = k < nd; }
                else { const int s = st_kmer_shift(prev, cur, nkmer); pp += s; plain += s; }
                prev = cur;
            }
            if (k < nd) {
                if (pp == ppos) evdwell += w[u];
                else {
                    if (pp == ppos + 1 && cur + 1 != pstate) { tot += evdwell; nstep++; }
                    evdwell = w[u]; ppos = pp; pstate = cur + 1;
                }
            }
        }
    }
    if (prev < 0) { a.blen[rd] = -1; a.redo[rd] = 0; return -1; }      /* every entry a stay: no call */
    const float prior = __fdiv_rn(d.prior_num[rd], (float)plain);
    const float scale = (float)__ddiv_rn((double)__fadd_rn(prior, (float)tot), 1.0 + (double)nstep);

    /* sweep two */
    unsigned *out32 = (unsigned *)(a.bases + a.bases_off[rd]);
    int *pos = a.pos ? a.pos + a.seq_off[rd] : nullptr;
    const int cap = d.cap[rd];
    unsigned word = 0;
    int nout = 0;
    bool over = false;
    auto emit = [&](int base) {
        word |= ((0x54474341u >> (8 * (base & 3))) & 0xffu) << (8 * (nout & 3));      /* 'A' 'C' 'G' 'T' */
        if ((++nout & 3) == 0) { if (nout <= cap) out32[(nout >> 2) - 1] = word; else over = true; word = 0; }
    };
    auto run = [&](int base, int hdwell, int less) {       /* a homopolymer's bases (the last one's: one less, decode.c:633-635) */
        const float q = roundf(__fdiv_rn((float)hdwell, scale));
        if (!(q >= 0.0f && q <= (float)(cap - nout))) { over = true; return; }
        for (int i = (int)q - less; i > 0; i--) emit(base);
    };
    prev = -1; pp = 0;
    int homo = -1, hd = 0;
    for (int k0 = 0; k0 < n && !over; k0 += 8) {
        int v[8], w[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { v[u] = SQ(min(k0 + u, n - 1)); w[u] = dw[min(k0 + u, nd - 1)]; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int k = k0 + u, cur = v[u];
            if (k >= n) break;
            if (cur >= 0) {
                int s = 0;
                if (prev >= 0) { s = st_kmer_shift(prev, cur, nkmer); pp += s; }
                if (prev < 0) { if (k < nd || !corr) for (int i = klen - 1; i >= 0; i--) emit(cur >> (2 * i)); }
                else if (k < nd && corr) {
                    if (cur == homo) hd += w[u];                            /* a repeat of the homopolymer's k-mer: dwell, no base */
                    else {
                        if (homo >= 0) { run(homo, hd, 0); homo = -1; hd = 0; }
                        for (int i = s - 1; i >= 0; i--) emit(cur >> (2 * i));
                        if (cur == st_repeat_kmer(cur & 3, klen)) { homo = cur; hd = w[u]; }      /* entered behind the first k-mer only */
                    }
                }
                prev = cur;
            } else if (homo >= 0 && k < nd) hd += w[u];                    /* a stay inside a homopolymer */
            if (pos) PS(k) = pp;
        }
    }
    if (homo >= 0 && !over) run(homo, hd, 1);
    if ((nout & 3) && !over) { if (((nout + 3) & ~3) <= cap) out32[nout >> 2] = word; else over = true; }
#undef SQ
#undef PS
    a.redo[rd] = over ? 1u : 0u;
    a.blen[rd] = over ? 0 : nout;
    return over ? 0 : nout;
}

/* stitching alone (k_stitch's place: behind k_backtrace where the tail runs as three kernels, and the test hook) */
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(SH_STITCH_VGPR_HALF))) void k_stitch_dwell(ShStitchArgs a, ShDwellArgs d) {
    const int rd = blockIdx.x * blockDim.x + threadIdx.x;
    if (rd >= a.npad) return;
    (void)dwell_read(a, d, rd);
}

/* k_walk_stitch_out with the dwell correction for the stitching: walk back, stitch, results to pinned host memory by the wave */
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(SH_STITCH_VGPR_HALF))) void k_walk_dwell_out(ShWalkArgs w, ShStitchArgs a, ShDwellArgs d, ShResultArgs r, ShMeta md) {
    const int rd0 = blockIdx.x * 64, lane = threadIdx.x;
    const int rd = rd0 + lane;
    int mylen = -1;
    if (rd < a.npad) {
        backtrace_read(w.tb, w.tb_end, w.final_state, md, w.seq_off, w.seq, rd, w.NQ, a.sstride);
        mylen = dwell_read(a, d, rd);
        r.h_blen[rd] = mylen; r.h_redo[rd] = a.redo[rd]; r.h_score[rd] = r.d_score[rd]; r.h_bad[rd] = r.d_bad[rd];
        if (rd == 0) *r.h_err = *r.d_err;
    }
    __syncthreads();                               /* the lanes' bases (global stores) are the wave's to read */
    const int nrd = min(64, a.npad - rd0);
    for (int k = 0; k < nrd; k++) {
        const int len = __shfl(mylen, k);
        if (len <= 0) continue;
        const u32x4 *src = (const u32x4 *)(r.d_bases + r.bases_off[rd0 + k]);
        u32x4 *dst = (u32x4 *)(r.h_bases + r.bases_off[rd0 + k]);
        for (int i = lane; i < (len + 15) / 16; i += 64) dst[i] = src[i];
    }
}

#endif /* SH_DWELL_H */
