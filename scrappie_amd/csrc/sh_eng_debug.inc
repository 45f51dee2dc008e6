/* sh_eng_debug.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * measurement / test hooks: decoder and trunk inputs, debug_option / debug_fetch / debug_stitch / debug_stitch_dwell / debug_split / debug_gates. */

extern "C" int scrappie_hip_set_decoder_input(scrappie_hip_engine *e, const float *d_prob, const uint64_t *prob_off, size_t n_prob) {
    if (!e) return set_err("set_decoder_input: null engine");
    if (e->any_pending()) return set_err("set_decoder_input: launch groups are in flight");
    return e->alt_prob.set("set_decoder_input", d_prob, prob_off, n_prob);
}

extern "C" int scrappie_hip_set_trunk_input(scrappie_hip_engine *e, const float *d_trunk, const uint64_t *trunk_off, size_t n_trunk) {
    if (!e) return set_err("set_trunk_input: null engine");
    if (e->any_pending()) return set_err("set_trunk_input: launch groups are in flight");
    return e->alt_trunk.set("set_trunk_input", d_trunk, trunk_off, n_trunk);
}

static scrappie_hip_engine *default_engine();      /* (sh_eng_surface.inc) */

/* Test hooks.  Options: "ff_separate" (S1 and the decoder as two kernels on this engine, whatever the shape),
 * "dump_final" (the decoders leave every tile's final scores, start and end state in the hand-over buffer). */
extern "C" int scrappie_hip_debug_option(scrappie_hip_engine *e, const char *name, int value) {
    if (!e && name && (!strcmp(name, "map_pack_cells") || !strcmp(name, "map_crf_local_stride") || !strcmp(name, "map_local_stride") || !strcmp(name, "crf_find_cells") || !strcmp(name, "map_crf_pack_cells") || !strcmp(name, "squig_pack_cells") || !strcmp(name, "squig_pack_lone") || !strcmp(name, "squig_local_stride") || !strcmp(name, "map_edits_band_width"))) e = default_engine();      /* the per-read surface's engine has no handle */
    if (!e || !name) return set_err("debug_option: null argument");
    if (e->any_pending()) return set_err("debug_option: launch groups are in flight");
    if (!strcmp(name, "ff_separate")) e->dbg_ff_separate = value != 0;
    else if (!strcmp(name, "fv_single")) e->dbg_fv_single = value != 0;
    else if (!strcmp(name, "dump_final")) e->dbg_dump_final = value != 0;
    else if (!strcmp(name, "fail_run")) e->dbg_fail_run = value;
    else if (!strcmp(name, "redo_all")) e->dbg_redo_all = value != 0;
    else if (!strcmp(name, "dwell_tight")) e->dbg_dwell_tight = value != 0;
    else if (!strcmp(name, "gru_tiles")) e->dbg_gru_tiles = value;
    else if (!strcmp(name, "decoder_cus")) e->dbg_decoder_cus = value > 0 ? value : 0;      /* the decoder's piece schedule believes the device has this many CUs (0: its own count) */
    else if (!strcmp(name, "decoder_lanes")) e->dbg_decoder_lanes = value > 0 ? value : 0;  /* the two-team decoder's lane layout believes the device has this many CUs (0: its own count) */
    else if (!strcmp(name, "force_f32_layers")) e->dbg_force_f32 = value != 0;
#ifdef SH_EXPERIMENTS
    else if (!strcmp(name, "gru32")) e->dbg_gru32 = value;
#endif
    else if (!strcmp(name, "tail")) e->tail_mode = value;
    else if (!strcmp(name, "fail_tail")) e->dbg_fail_tail = value;
    else if (!strcmp(name, "tail_free_frac")) e->dbg_tail_free_frac = value / 1000.0;      /* what the helper engine's creation takes for the device's free share (in 1/1000) */
    else if (!strcmp(name, "squiggle_budget_kb")) e->dbg_squig_budget = value > 0 ? (size_t)value << 10 : 0;      /* device bytes per squiggle-matching launch (0: from free memory) */
    else if (!strcmp(name, "sqnet_budget_kb")) e->dbg_sqnet_budget = value > 0 ? (size_t)value << 10 : 0;      /* device bytes per squiggle-predicting launch (0: from free memory) */
    else if (!strcmp(name, "map_pack_cells")) e->map_pack.cells = value < 0 ? -1 : value;      /* cells per pack of candidates (0: every candidate through k_map; -1: the default) */
    else if (!strcmp(name, "map_crf_local_stride")) e->map_crf_local_stride = value < 0 ? -1 : value;      /* start cells per window of k_map_crf_local (0: one window; -1: the default) */
    else if (!strcmp(name, "map_local_stride")) e->map_local_stride = value < 0 ? -1 : value;      /* entry positions per window of k_map_local (0: one window; -1: the default) */
    else if (!strcmp(name, "crf_find_cells")) e->crf_find_cells = value < 0 ? -1 : value;      /* cells per pack of motifs of k_crf_find (-1: the default) */
    else if (!strcmp(name, "map_crf_pack_cells")) e->map_crf_pack.cells = value < 0 ? -1 : value;      /* cells per pack of candidates of k_map_crf_pack (0: every candidate through k_map_crf; -1: the default) */
    else if (!strcmp(name, "squig_local_stride")) e->squig_local_stride = value < 0 ? -1 : value;      /* entry positions per window of k_squig_local (0: one window; -1: the default) */
    else if (!strcmp(name, "squig_pack_cells")) e->squig_pack_cells = value < 0 ? -1 : value;      /* cells per pack of candidate squiggles of k_squig_pack (0: every candidate through k_squig; -1: the default) */
    else if (!strcmp(name, "squig_pack_lone")) e->squig_pack_lone = value != 0;      /* 1: a candidate alone in its pack runs in k_squig_pack (0, the default: it takes k_squig) */
    else if (!strcmp(name, "crf_edits_budget_kb")) e->crf_edits.budget = value > 0 ? (size_t)value << 10 : 0;      /* row and result bytes per launch of the three edit kernels (0: one launch per launch group) */
    else if (!strcmp(name, "map_edits_budget_kb")) e->map_edits.budget = value > 0 ? (size_t)value << 10 : 0;      /* the same for the three transducer edit kernels */
    else if (!strcmp(name, "map_edits_band_width")) {        /* positions per workgroup of the banded k_map_edits: 64 or 256 (0: the default of the form) */
        if (value != 0 && value != 64 && value != 256) return set_err("debug_option: map_edits_band_width is 0 (the default), 64 or 256");
        e->map_edits_band_width = value;
    }
    else if (!strcmp(name, "events_budget_samples")) e->dbg_events_budget = value > 0 ? (size_t)value : 0;      /* sample slots per event-detection launch (0: from free memory) */
    else return set_err("debug_option: unknown option '%s'", name);
    return 0;
}

/* Copy a device buffer of the most recent transducer launch group to the host (everything in flight is drained
 * first): "tb" (one byte per state: [column block][quad][read of tile][state of quad]), "tb_end" (int per column
 * block and read), "final_state" (int per read, tiled order), "final_score" (float per read, tiled order),
 * "final_scores" ([tile][states x 16 reads + 16 start + 16 end] floats; needs the dump_final option),
 * "order" (int per tiled position: index of the read in the call, -1 = padding), "tile_boff" (long long per tile),
 * "n_redo" (unsigned long long: reads k_stitch has left to the host since the engine was created), "gru_tiles" (int:
 * tiles per workgroup of the group's recurrent layers, 1 or 2), "decoder_pieces" (int: segments of tiles the group's decoder launch ran -- one per workgroup for the
 * kernels that own a piece of a tile, all the segments its workgroups walked for the two-team kernel's lane layout; the "decoder_cus" and
 * "decoder_lanes" options cut small groups), "decoder_wgs" (int: workgroups of that launch).
 * Returns the number of bytes the buffer holds (copies min(that, nbytes)), -1 on error. */
extern "C" long long scrappie_hip_debug_fetch(scrappie_hip_engine *e, const char *what, void *dst, size_t nbytes) {
    if (!e || !what) return set_err("debug_fetch: null argument");
    (void)hipSetDevice(e->device);
    HIPCHK(sh_stream_wait(e->stream));
    HIPCHK(sh_stream_wait(e->cstream));
    const Slot &sl = e->current(); const LaunchGroup &lg = sl.lg;
    if (!lg.valid) return set_err("debug_fetch: no launch group has run");
    Model *m = get_model(e, lg.model);
    if (!m) return -1;
    const size_t NH = (size_t)std::max(m->NS - 1, 0);
    const void *src = nullptr; size_t have = 0; bool host = false;
    const int gru_tiles = lg.gru_two ? 2 : 1;
    if (!strcmp(what, "tb")) { src = e->d_tb.p; have = (size_t)lg.ncb * NH * 16; }
    else if (!strcmp(what, "tb_end")) { src = e->d_tbend.p; have = (size_t)lg.ncb * 16 * 4; }
    else if (!strcmp(what, "final_state")) { src = e->d_fstate.p; have = lg.npad * 4; }
    else if (!strcmp(what, "final_score")) { src = sl.d_fscore.p; have = lg.npad * 4; }
    else if (!strcmp(what, "final_scores")) { src = e->d_vstate.p; have = lg.ntile * (NH * 16 + 32) * 4; }
    else if (!strcmp(what, "order")) { src = lg.order.data(); have = lg.npad * 4; host = true; }
    else if (!strcmp(what, "tile_boff")) { src = lg.tile_boff.data(); have = lg.ntile * 8; host = true; }
    else if (!strcmp(what, "n_redo")) { static thread_local unsigned long long tot; tot = e->n_redo + e->n_redo_tail; src = &tot; have = 8; host = true; }
    else if (!strcmp(what, "n_tail_groups")) { src = &e->n_tail_groups; have = 8; host = true; }
    else if (!strcmp(what, "n_tail_calls")) { src = &e->n_tail_calls; have = 8; host = true; }
    else if (!strcmp(what, "n_tail_reads")) { src = &e->n_tail_reads; have = 8; host = true; }
    else if (!strcmp(what, "gru_tiles")) { src = &gru_tiles; have = 4; host = true; }
    else if (!strcmp(what, "decoder_pieces")) { src = &lg.vit_launched; have = 4; host = true; }
    else if (!strcmp(what, "decoder_wgs")) { src = &lg.vit_launched_wg; have = 4; host = true; }
    else if (!strcmp(what, "pinned_bytes")) {      /* pinned host memory this engine holds (staging, results, metadata; both slots) */
        static thread_local unsigned long long tot;
        tot = e->slots[0].pinned_bytes() + e->slots[1].pinned_bytes();
        src = &tot; have = 8; host = true;
    }
    else return set_err("debug_fetch: unknown buffer '%s'", what);
    if (!src && have) return set_err("debug_fetch: buffer '%s' was not allocated", what);
    const size_t cnt = std::min(have, nbytes);
    if (dst && cnt) {
        if (host) memcpy(dst, src, cnt);
        else HIPCHK(hipMemcpy(dst, src, cnt, hipMemcpyDeviceToHost));
    }
    return (long long)have;
}

/* k_stitch on ONE read given on the host (test hook: the device form of homopolymer_path + overlapper /
 * crfpath_to_basecall against the compiled-reference fixtures).  path: nblock + 1 entries; side: [nblock][5] log-
 * posterior rows (homopolymer k-mers of A, C, G, T, stay) or NULL (no homopolymer pass); nstate: 4^k + 1, or 25 with
 * crf != 0.  bases gets at most cap bytes incl. the NUL; pos (nblock + 1 ints) and redo (1: the device left the
 * decision to the host) may be NULL.  Returns the number of bases, -1 = no call, -2 = error. */
extern "C" long scrappie_hip_debug_stitch(scrappie_hip_engine *e, const int *path, const float *side, size_t nblock, int nstate, int crf,
                                          char *bases, size_t cap, int *pos, int *redo) {
    if (!e || !path || !bases || nblock == 0) { set_err("debug_stitch: bad argument"); return -2; }
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t T = nblock, npad = 64, bcap = 5 * (T + 1) + 8;
    DBuf dmeta, dseq, dhp, dpos, dbases, dblen, dredo;      /* (freed on every way out) */
    /* metadata of a group of one read: [seq_off | hp_off | bases_off] (long long x npad each), rT (int x npad) */
    std::vector<char> hm(npad * 8 * 3 + npad * 4, 0);
    int *rT = (int *)(hm.data() + npad * 24);
    rT[0] = (int)T;
    if (dmeta.ensure(hm.size()) || dseq.ensure((T + 1) * 4) || dpos.ensure((T + 1) * 4) || dbases.ensure(bcap) ||
        dblen.ensure(npad * 4) || dredo.ensure(npad * 4) || (side && dhp.ensure(T * 5 * 4))) return -2;
    hipStream_t s = e->stream;
    if (hipMemcpyAsync(dmeta.p, hm.data(), hm.size(), hipMemcpyHostToDevice, s) != hipSuccess) return -2;
    if (hipMemcpyAsync(dseq.p, path, (T + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess) return -2;
    if (side && hipMemcpyAsync(dhp.p, side, T * 5 * 4, hipMemcpyHostToDevice, s) != hipSuccess) return -2;
    if (hipMemsetAsync(dredo.p, 0, npad * 4, s) != hipSuccess) return -2;
    if (sh_stream_wait(s) != hipSuccess) return -2;                 /* sources are pageable caller memory */
    char *d = dmeta.as<char>();
    ShMeta md{};
    md.rT = (const int *)(d + npad * 24);
    ShStitchArgs sa;
    sa.seq = dseq.as<int>(); sa.seq_off = (const long long *)d;
    sa.hp = side ? dhp.as<float>() : nullptr; sa.hp_off = (const long long *)(d + npad * 8);
    sa.pos = pos ? dpos.as<int>() : nullptr;
    sa.bases = dbases.as<char>(); sa.bases_off = (const long long *)(d + npad * 16);
    sa.blen = dblen.as<int>(); sa.redo = dredo.as<unsigned>();
    sa.npad = 1; sa.nstate = nstate; sa.crf = crf; sa.sstride = 1;
    hipLaunchKernelGGL(k_stitch, dim3(1), dim3(64), 0, s, sa, md);
    int len = -1; unsigned rd = 0;
    if (hipMemcpyAsync(&len, dblen.p, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return -2;
    if (hipMemcpyAsync(&rd, dredo.p, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return -2;
    if (sh_stream_wait(s) != hipSuccess) { set_err("debug_stitch: %s", hipGetErrorString(hipGetLastError())); return -2; }
    if (redo) *redo = (int)rd;
    if (len >= 0) {
        if ((size_t)len + 1 > cap) { set_err("debug_stitch: %d bases do not fit %zu bytes", len, cap); return -2; }
        if (len && hipMemcpy(bases, dbases.p, (size_t)len, hipMemcpyDeviceToHost) != hipSuccess) return -2;
        bases[len] = 0;
        if (pos && !crf && hipMemcpy(pos, dpos.p, (T + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    }
    return len;
}

/* k_stitch_dwell on a batch of reads given on the host (test hook: the device form of the dwell correction against the compiled-reference
 * fixtures and the host statement).  One launch, 64 reads to a wave; see include/scrappie_hip.h for the layout. */
extern "C" int scrappie_hip_debug_stitch_dwell(scrappie_hip_engine *e, const int *paths, const int *dwells, const size_t *nentry, size_t nread, int ntrail,
                                               const float *prior_num, int nstate, const size_t *cap, char *bases, size_t bases_bytes, int *lengths, int *pos,
                                               int *redo) {
    if (!e || !paths || !dwells || !nentry || !prior_num || !cap || !bases || !lengths || nread == 0 || nread > (1u << 20) || (ntrail != 0 && ntrail != 1))
        return set_err("debug_stitch_dwell: bad argument");
    if (nstate != 5 && nstate != 17 && nstate != 65 && nstate != 257 && nstate != 1025) return set_err("debug_stitch_dwell: %d states (4^k + 1 with k <= 5)", nstate);
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t npad = (nread + 63) / 64 * 64;
    /* per-read words: [seq_off | bases_off | dwell_off] (long long x npad each), prior_num (float x npad), nd, cap (int x npad each) */
    std::vector<char> hm(npad * 36, 0);
    long long *seq_off = (long long *)hm.data(), *bases_off = seq_off + npad, *dwell_off = bases_off + npad;
    float *num = (float *)(dwell_off + npad);
    int *nd = (int *)(num + npad), *capi = nd + npad;
    size_t nseq = 0, ndw = 0, nb = 0;
    for (size_t i = 0; i < nread; i++) {
        const size_t c = (cap[i] + 15) & ~(size_t)15;
        if (nentry[i] == 0 || nentry[i] > (1u << 28) || c == 0 || c > (1u << 30)) return set_err("debug_stitch_dwell: read %zu: %zu entries, %zu bytes", i, nentry[i], cap[i]);
        seq_off[i] = (long long)nseq; nseq += nentry[i] + (size_t)ntrail;
        dwell_off[i] = (long long)ndw; ndw += nentry[i];
        bases_off[i] = (long long)nb; nb += c;
        num[i] = prior_num[i]; nd[i] = (int)nentry[i]; capi[i] = (int)c;
    }
    if (nb > bases_bytes) return set_err("debug_stitch_dwell: the reservations take %zu bytes, bases holds %zu", nb, bases_bytes);
    DBuf dmeta, dseq, ddw, dpos, dbases, dblen, dredo;      /* (freed on every way out) */
    if (dmeta.ensure(hm.size()) || dseq.ensure(nseq * 4) || ddw.ensure(ndw * 4) || dpos.ensure(nseq * 4) || dbases.ensure(nb) ||
        dblen.ensure(npad * 4) || dredo.ensure(npad * 4)) return -1;
    hipStream_t s = e->stream;
    HIPCHK(hipMemcpyAsync(dmeta.p, hm.data(), hm.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dseq.p, paths, nseq * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ddw.p, dwells, ndw * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dbases.p, 0, nb, s));
    HIPCHK(hipMemsetAsync(dpos.p, 0, nseq * 4, s));
    HIPCHK(hipMemsetAsync(dredo.p, 0, npad * 4, s));
    HIPCHK(sh_stream_wait(s));                      /* sources are pageable caller memory */
    char *d = dmeta.as<char>();
    ShStitchArgs sa{};
    sa.seq = dseq.as<int>(); sa.seq_off = (const long long *)d;
    sa.hp = nullptr; sa.hp_off = nullptr;
    sa.pos = pos ? dpos.as<int>() : nullptr;
    sa.bases = dbases.as<char>(); sa.bases_off = (const long long *)(d + npad * 8);
    sa.blen = dblen.as<int>(); sa.redo = dredo.as<unsigned>();
    sa.npad = (int)nread; sa.nstate = nstate; sa.crf = 0; sa.sstride = 1;
    ShDwellArgs da{};
    da.dwell = ddw.as<int>(); da.dwell_off = (const long long *)(d + npad * 16);
    da.prior_num = (const float *)(d + npad * 24);
    da.nd = (const int *)(d + npad * 28); da.cap = (const int *)(d + npad * 32);
    da.ntrail = ntrail;
    hipLaunchKernelGGL(k_stitch_dwell, dim3((unsigned)(npad / 64)), dim3(64), 0, s, sa, da);
    HIPCHK(hipGetLastError());
    std::vector<unsigned> hredo(nread);
    HIPCHK(hipMemcpyAsync(lengths, dblen.p, nread * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hredo.data(), dredo.p, nread * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(bases, dbases.p, nb, hipMemcpyDeviceToHost, s));
    if (pos) HIPCHK(hipMemcpyAsync(pos, dpos.p, nseq * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    if (redo) for (size_t i = 0; i < nread; i++) redo[i] = (int)hredo[i];
    return 0;
}

/* split8 (sh_kernels.h: the cut every split product's activations go through) on consecutive groups of eight values */
__global__ void k_debug_split(const float *x, unsigned *p1, unsigned *p2, size_t ngroup) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroup) return;
    const ShSplit sp = split8(*(const f32x4 *)(x + g * 8), *(const f32x4 *)(x + g * 8 + 4));
    *(u32x4 *)(p1 + g * 4) = __builtin_bit_cast(u32x4, sp.p1);
    *(u32x4 *)(p2 + g * 4) = __builtin_bit_cast(u32x4, sp.p2);
}

/* The two fp16 pieces of n values given on the host, as the kernels cut them (test hook: the device's cut against its
 * definition, bit for bit).  p1 and p2 take n fp16 bit patterns each.  Returns 0, -1 on error. */
extern "C" int scrappie_hip_debug_split(scrappie_hip_engine *e, const float *x, size_t n, uint16_t *p1, uint16_t *p2) {
    if (!e || !x || !p1 || !p2 || n == 0 || n > ((size_t)1 << 30)) return set_err("debug_split: bad argument");
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t ngroup = (n + 7) / 8, npad = ngroup * 8;      /* the last group is filled with zeros */
    DBuf dx, d1, d2;      /* (freed on every way out) */
    if (dx.ensure(npad * 4) || d1.ensure(npad * 2) || d2.ensure(npad * 2)) return -1;
    hipStream_t s = e->stream;
    HIPCHK(hipMemsetAsync(dx.p, 0, npad * 4, s));
    HIPCHK(hipMemcpyAsync(dx.p, x, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(sh_stream_wait(s));                      /* the source is pageable caller memory */
    hipLaunchKernelGGL(k_debug_split, dim3((unsigned)((ngroup + 255) / 256)), dim3(256), 0, s, dx.as<float>(), d1.as<unsigned>(), d2.as<unsigned>(), ngroup);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(p1, d1.p, n * 2, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(p2, d2.p, n * 2, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    return 0;
}

/* one of the activation forms of sh_kernels.h on consecutive groups of four values (`which`: scrappie_hip.h, SH_GATE_*) */
__global__ void k_debug_gates(int which, const float *x, float *y, size_t ngroup) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroup) return;
    const f32x4 v = *(const f32x4 *)(x + g * 4);
    f32x4 r = v;
    switch (which) {
    case SH_GATE_LOGISTIC:
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = d_logistic(v[k]);
        break;
    case SH_GATE_TANH:
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = d_tanh(v[k]);
        break;
    case SH_GATE_LOGISTIC4: r = d_logistic4(v); break;
    case SH_GATE_TANH4: r = d_tanh4(v); break;
    case SH_GATE_LOGISTIC4_ACC: r = d_logistic4_acc(v); break;
    case SH_GATE_TANH4_ACC: r = d_tanh4_acc(v); break;
    case SH_GATE_EXP:
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = d_exp(v[k]);
        break;
    case SH_GATE_EXP_ACC:
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = d_exp_acc(v[k]);
        break;
    case SH_GATE_EXP_ACC_INRANGE:
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = d_exp_acc_inrange(v[k]);
        break;
    default:
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = d_elu(v[k]);
        break;
    }
    *(f32x4 *)(y + g * 4) = r;
}

/* One activation form of the kernels on n values given on the host (test hook: the forms against each other bit for bit, and against
 * float64, outside the range network weights reach).  The _ACC forms take their argument in accumulator units (2^14 x).  Returns 0, -1 on error. */
extern "C" int scrappie_hip_debug_gates(scrappie_hip_engine *e, int which, const float *x, size_t n, float *out) {
    if (!e || !x || !out || n == 0 || n > ((size_t)1 << 30) || which < 0 || which >= SH_GATE_NFORM) return set_err("debug_gates: bad argument");
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t ngroup = (n + 3) / 4, npad = ngroup * 4;      /* the last group is filled with zeros */
    DBuf dx, dy;      /* (freed on every way out) */
    if (dx.ensure(npad * 4) || dy.ensure(npad * 4)) return -1;
    hipStream_t s = e->stream;
    HIPCHK(hipMemsetAsync(dx.p, 0, npad * 4, s));
    HIPCHK(hipMemcpyAsync(dx.p, x, n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(sh_stream_wait(s));                      /* the source is pageable caller memory */
    hipLaunchKernelGGL(k_debug_gates, dim3((unsigned)((ngroup + 255) / 256)), dim3(256), 0, s, which, dx.as<float>(), dy.as<float>(), ngroup);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dy.p, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    return 0;
}

extern "C" void scrappie_hip_free_calls(scrappie_hip_call *calls, size_t n) {
    if (!calls) return;
    for (size_t i = 0; i < n; i++) { free(calls[i].basecall); free(calls[i].pos); calls[i].basecall = nullptr; calls[i].pos = nullptr; }
}
