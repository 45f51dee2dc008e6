/* sh_eng_pipeline.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * run_pipeline: one launch group through its kernels, stage by stage. */

/* ------------------------------------------------------------------ */
/* the device pipeline                                                  */
/* ------------------------------------------------------------------ */
enum StopAt { STOP_NONE = 0, STOP_TRUNK = 1, STOP_POST = 2 };

struct RunOut {   /* where things are on the device after a run */
    const float *act = nullptr;   /* trunk output [ncb][S/16][256] */
    int act_units = 0;
    const float *E = nullptr;     /* transducer: exp values; rnnrf: normalised transitions */
    const float *sums = nullptr;
};

/* SH_HOST_STAMP: host-side wall time since the stamp was made, on stderr */
struct HostStamp {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what, const char *after = "") const {
        if (tun().host_stamp) fprintf(stderr, "host stamp: %s %.2f ms%s\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), after);
    }
};

/* Profiling marks of one launch group: mark() records the slot's next event on a stream (nothing when profiling is off or the slot's 48 events are
 * used up), span() books the time between two marks to a field of scrappie_hip_timing (resolve_spans reads the events once the group is done).  The
 * marks of a layer are recorded again by every layer: a span holds the events its marks had when it was booked. */
struct Marks {
    enum Mark { PROLOGUE_BEGIN, PROLOGUE_END,      /* prologue stream */
                WAIT_BEGIN, MAIN_BEGIN,            /* main stream: in front of and behind its wait for the prologue */
                LAYER_BEGIN, LAYER_SPLIT, LAYER_END,       /* projection | recurrence (one kernel: everything behind LAYER_SPLIT) */
                S1_BEGIN, S1_END, DECODE_END, MAIN_END,
                WALK_BEGIN, WALK_END, STITCH_BEGIN, STITCH_END,    /* copy stream */
                N_MARKS };
    Slot *sl = nullptr;
    bool on = false;
    int at[N_MARKS] = {0};
    int mark(Mark k, hipStream_t st) {
        if (on && sl->nev < 48) { at[k] = sl->nev++; HIPCHK(hipEventRecord(sl->ev[at[k]], st)); }
        return 0;
    }
    void span(SpanField field, Mark from, Mark to) { if (on) sl->spans.push_back({field, at[from], at[to]}); }
};

/* what the stages of one launch group share */
struct GroupRun {
    scrappie_hip_engine *e = nullptr;
    const float *d_signal = nullptr; const uint64_t *offsets = nullptr; const scrappie_hip_params *p = nullptr;
    StopAt stop = STOP_NONE; int trunk_upto = 5; RunOut *ro = nullptr;
    bool transducer = false, hp_on = false;
    const DwellJob *dw = nullptr;      /* events with the dwell correction: the group's dwells (null: plain stitching) */
    const PostJob *pj = nullptr;       /* flip-flop models: base probabilities wanted, and where they go (null: none) */
    MetaPtrs mp;
    hipStream_t s = nullptr, ps = nullptr, cs = nullptr;      /* main, prologue and copy stream (all three the main stream where the engine has no events) */
    long long ncb = 0; size_t act_bytes = 0;
    float *abuf[3] = {nullptr, nullptr, nullptr};      /* the slot's convolution output, the layers' two shared buffers */
    bool fuse_conv = false;       /* experiment: the first recurrent layer computes the convolution itself */
    bool walk_on_cs = false;      /* the traceback walk runs on the copy stream */
    bool fold_tail = false;       /* ... as part of k_walk_stitch_out */
    Marks pf;
    HostStamp stamp;
};

static int crf_post_mark(Slot &sl, int k, hipStream_t st);
static int crf_post_enqueue(Slot &sl, GroupRun &c);      /* sh_eng_crfpost.inc */
static int crf_post_download(Slot &sl, GroupRun &c);

static int longest_tile(const LaunchGroup &lg) {      /* sorted: the first read of a tile is its longest */
    int maxT = 0;
    for (size_t i = 0; i < lg.npad; i += 16) maxT = std::max(maxT, lg.rT[i]);
    return maxT;
}

/* a group has been enqueued as far as its caller wanted it */
static void mark_pending(scrappie_hip_engine *e, Slot &sl) {
    sl.pending = true;
    if (!e->other(sl).pending) e->oldest = e->index(sl);
}

/* Stage 0: take a free slot (a slot stays taken until scrappie_hip_collect picks it up) and lay the group out in it.  *empty: no read of the group
 * is long enough to run, and the group is complete as it stands. */
static int begin_group(scrappie_hip_engine *e, Model *m, const uint32_t *lengths, size_t n, GroupRun &c, Slot **slot, bool *empty) {
    Slot *slp = nullptr;
    for (int k = 0; k < 2 && !slp; k++) { Slot &cand = e->slots[(e->cur + 1 + k) & 1]; if (!cand.pending) slp = &cand; }
    if (!slp) return set_err("two launch groups are already in flight: call scrappie_hip_collect first");
    Slot &sl = *slp;
    e->cur = e->index(sl);
    if (build_group(e, sl, m, c.offsets, lengths, n, c.hp_on, c.mp, c.dw, c.pj)) return -1;
    c.stamp("build_group");
    *slot = slp;
    *empty = sl.lg.ncb == 0;
    if (*empty) {
        sl.lg.valid = true; sl.lg.model = (int)(std::find(e->models.begin(), e->models.end(), m) - e->models.begin());
        if (c.stop == STOP_NONE) { if (e->ev_ok) HIPCHK(hipEventRecord(sl.done, c.s)); mark_pending(e, sl); }
    }
    return 0;
}

/* Stage 1, on its own (low-priority) stream: metadata and flag clears (build_group) and the convolution.  Nothing in it
 * depends on the previous launch group, and k_conv_act is built to fit beside k_gru_proj's waves (32 of the 512 VGPRs
 * of a SIMD stay free next to three of them), so while group k walks its recurrent layers the convolution of group
 * k + 1 is already running; the main stream only waits for it.  Its output has a buffer per slot. */
static int stage_prologue(Slot &sl, Model *m, GroupRun &c) {
    scrappie_hip_engine *e = c.e;
    LaunchGroup &lg = sl.lg;
    const hipStream_t s = c.s; hipStream_t &ps = c.ps;
    const int F = m->F;
#ifdef SH_EXPERIMENTS
    static const bool rnnrf_main = getenv("SH_RNNRF_CONV_MAIN") != nullptr;
#else
    const bool rnnrf_main = false;
#endif
    if (e->ev_ok && m->arch == 1 && rnnrf_main) {
        /* experiment switch: rnnrf's convolution on the main stream.  With the VALU form of the convolution that was the
         * better place for this model (a step of 19 ms, 80 % of it recurrent layers: 19.33 against 19.65 ms); with
         * k_conv_mfma the prologue stream wins there too (19.75 against 20.1 ms on one box) */
        HIPCHK(hipEventRecord(sl.pdone, ps)); HIPCHK(hipStreamWaitEvent(s, sl.pdone, 0));
        ps = s;
    }
    if (sl.d_conv.ensure(c.act_bytes)) return -1;
    c.abuf[0] = sl.d_conv.as<float>(); c.abuf[1] = e->d_act[1].as<float>(); c.abuf[2] = e->d_act[2].as<float>();
    /* SH_CONV_IN_LAYER=1 (experiment; identical results, measured slower: DESIGN.md section 5): the convolution inside the
     * first recurrent layer (k_gru_conv) where the whole path runs as a basecall of an rgrgr model of the shipped shape;
     * everywhere else (hooks that stop after a stage, other shapes, the two-kernel layer forms) it is a kernel of its own. */
    const int kst = (m->WL + 3) / 4;
#ifdef SH_EXPERIMENTS
    c.fuse_conv = tun().conv_in_layer && !tun().conv_valu && m->arch == 0 && F == 96 && m->S == 96 && (kst == 3 || kst == 5) &&
                  c.stop == STOP_NONE && c.trunk_upto >= 5 && !tun().gru_separate && !m->layer_f32[0] &&
                  !(SH_GRU_FREE_DEFAULT ? !tun().gru_barrier : tun().gru_free);
    if (c.fuse_conv) {
        if (sl.h_edge.ensure(lg.npad * 16) || sl.d_edge.ensure(lg.npad * 16)) return -1;
        int *ew = sl.h_edge.as<int>();
        for (size_t i = 0; i < lg.npad && c.fuse_conv; i++) {
            const int o = lg.order[i];
            if (!conv_edge_words(m->geom, lg.rN[i], lg.rT[i], ew + 4 * i)) c.fuse_conv = false;
            if (o >= 0 && lg.rT[i] > 0 && c.offsets[o] + (uint64_t)lg.rN[i] >= ((uint64_t)1 << 30)) c.fuse_conv = false;    /* 32-bit sample indices in the kernel */
        }
    }
#endif
    if (c.pf.mark(Marks::PROLOGUE_BEGIN, ps)) return -1;
    if (m->arch == 3) {   /* events: the input already is the feature matrix (12 floats per event) */
        dim3 grid((unsigned)lg.ntile, (unsigned)std::min(64, (longest_tile(lg) + 3) / 4));
        hipLaunchKernelGGL(k_feat_in, grid, dim3(256), 0, ps, c.d_signal, c.mp.md, m->nfeat, c.abuf[0], c.ncb, sl.d_bad.as<unsigned>());
    } else if (c.fuse_conv) {
        /* the first recurrent layer computes the convolution itself (k_gru_conv): what it needs to know about each read's
         * right edge goes to the device with the rest of the prologue */
        hipLaunchKernelGGL(k_upload_words, dim3((unsigned)std::min<size_t>((lg.npad + 255) / 256, 256)), dim3(256), 0, ps,
                           (const u32x4 *)sl.h_edge.p, sl.d_edge.as<u32x4>(), (long long)lg.npad);
    } else {   /* C1 + A1 */
        const int tchunk = tun().conv_tchunk;
        dim3 grid((unsigned)lg.ntile, (unsigned)std::min(65535, (longest_tile(lg) + tchunk - 1) / tchunk));   /* the kernel strides over y */
        /* something to run under (the other slot's group is in flight): the 48-register build; else the fast one */
        const bool bg = e->ev_ok && e->other(sl).pending && ps != s;
#ifdef SH_EXPERIMENTS
        static const int fake = getenv("SH_CONV_FAKE") ? atoi(getenv("SH_CONV_FAKE")) : 0;   /* experiment: 1 = a 3 GB fill instead of the convolution, 2 = nothing (results invalid) */
#else
        const int fake = 0;
#endif
        /* on the matrix pipe (k_conv_mfma) for the shapes of the shipped models: 96 filters, 11 or 19 taps */
        /* (one form per model, whichever stream it runs on: the two forms round differently, and a read's call must not depend
         * on whether its launch group had another one to run under) */
        const bool mfma_ok = !tun().conv_valu && F == 96 && (kst == 3 || kst == 5);
        const bool areg = kst == 3 && !bg;       /* taps in registers (70 VGPRs) when the kernel has the GPU to itself, from LDS (<= 56) beside k_gru_proj */
        const size_t lds = ((size_t)m->WL * F + F + (mfma_ok && !areg ? (size_t)6 * kst * 64 : 0) + 16 * ((size_t)(tchunk - 1) * m->stride + m->WL)) * 4;
        using ConvKernel = void (*)(const float *, ShMeta, const float *, const float *, ShConvGeom, float *, int, unsigned *);
        auto act = [&](ConvKernel none, ConvKernel tanh_) { return m->conv_act == 1 ? tanh_ : none; };
        const ConvKernel kern = !mfma_ok ? (bg ? act(k_conv_act_bg<0>, k_conv_act_bg<1>) : act(k_conv_act<0>, k_conv_act<1>))
                              : areg     ? act(k_conv_mfma<0, 6, 3, true>, k_conv_mfma<1, 6, 3, true>)       /* (never beside the layers: taps from LDS there) */
                              : kst == 3 ? (bg ? act(k_conv_mfma_bg<0, 6, 3, false>, k_conv_mfma_bg<1, 6, 3, false>) : act(k_conv_mfma<0, 6, 3, false>, k_conv_mfma<1, 6, 3, false>))
                                         : (bg ? act(k_conv_mfma_bg<0, 6, 5, false>, k_conv_mfma_bg<1, 6, 5, false>) : act(k_conv_mfma<0, 6, 5, false>, k_conv_mfma<1, 6, 5, false>));
        if (fake == 1) HIPCHK(hipMemsetAsync(c.abuf[0], 0, c.act_bytes, ps));
        else if (fake != 2) hipLaunchKernelGGL(kern, grid, dim3(256), lds, ps, c.d_signal, c.mp.md, m->conv_W.as<float>(), m->conv_b.as<float>(), m->geom, c.abuf[0], tchunk, sl.d_bad.as<unsigned>());
    }
    if (c.pf.mark(Marks::PROLOGUE_END, ps)) return -1;
    c.pf.span(F_CONV, Marks::PROLOGUE_BEGIN, Marks::PROLOGUE_END);
    c.stamp("prologue enqueued at");
    if (c.pf.mark(Marks::WAIT_BEGIN, s)) return -1;
    if (e->ev_ok && ps != s) { HIPCHK(hipEventRecord(sl.pdone, ps)); HIPCHK(hipStreamWaitEvent(s, sl.pdone, 0)); }
    c.stamp("wait enqueued at");
    if (c.pf.mark(Marks::MAIN_BEGIN, s)) return -1;                      /* the main stream's part of the group starts here */
    c.pf.span(F_WAIT, Marks::WAIT_BEGIN, Marks::MAIN_BEGIN); c.pf.span(F_LEAD, Marks::PROLOGUE_END, Marks::WAIT_BEGIN);
    if (tun().helper_fence && e->ev_ok && e->other(sl).pending) HIPCHK(hipStreamWaitEvent(s, e->other(sl).hdone, 0));
    return 0;
}

/* One recurrent layer l of I inputs, in -> out: GRU (three gates; rnnrf adds the input to the output) or, for the events model, peephole LSTM (four).
 * One kernel -- projection team + recurrence team per workgroup (k_gru_proj, k_lstm_proj) -- where the layer's shape allows; else the projection
 * (gate inputs through HBM) and the recurrence apart. */
static int recurrent_layer(Slot &sl, Model *m, GroupRun &c, int l, int I, const float *in, float *out, int backward) {
    scrappie_hip_engine *e = c.e;
    const LaunchGroup &lg = sl.lg; const MetaPtrs &mp = c.mp;
    const hipStream_t s = c.s;
    const bool lstm = m->arch == 3;
    const int S = m->S, gates = lstm ? 4 : 3;
    const float *resid = m->arch == 1 ? in : nullptr;
    const bool f32 = !lstm && m->layer_f32[l];            /* weights outside the split products' range: exact-fp32 kernels */
    const bool one_kernel = !tun().gru_separate && (lstm ? (I == S || I == 16) && S % 32 == 0 : gru_proj_ok(I, S) && !f32);
    if (c.pf.mark(Marks::LAYER_BEGIN, s)) return -1;
#ifdef SH_EXPERIMENTS
    if (l == 0 && c.fuse_conv) {
        if (c.pf.mark(Marks::LAYER_SPLIT, s)) return -1;
        ShConvFuse cf;
        cf.sig = c.d_signal; cf.W = m->conv_W.as<float>(); cf.bias = m->conv_b.as<float>(); cf.edge = sl.d_edge.as<int>();
        cf.bad = sl.d_bad.as<unsigned>(); cf.g = m->geom;
        if (launch_gru_conv(s, (m->WL + 3) / 4, m->conv_act, out, m->iWp[l].as<unsigned>(), m->ibs[l].as<float>(), m->sWp[l].as<unsigned>(),
                            m->sW2p[l].as<unsigned>(), mp.md, 1, mp.lanes1, lg.gru1_nwg, mp.lanes, lg.gru_nwg, lg.gru_two, cf)) return -1;
    } else if (!lstm && one_kernel && use_gru32(e) && S == 96 && I == 96 && m->has32) {
        if (c.pf.mark(Marks::LAYER_SPLIT, s)) return -1;
        if (use_gru32(e) == 2 ? launch_gru_proj32x2(s, in, out, m->arch == 1, m->iWp32[l].as<unsigned>(), m->ib32[l].as<float>(), m->sWp32[l].as<unsigned>(),
                                                    m->sW2p32[l].as<unsigned>(), mp.md, backward, mp.pairs2, lg.gru32x2_nwg, lg.ntile)
                              : launch_gru_proj32(s, in, out, m->arch == 1, m->iWp32[l].as<unsigned>(), m->ib32[l].as<float>(), m->sWp32[l].as<unsigned>(),
                                                  m->sW2p32[l].as<unsigned>(), mp.md, backward, mp.pairs, lg.gru32_nwg, lg.ntile)) return -1;
    } else
#endif
    if (one_kernel) {
        if (c.pf.mark(Marks::LAYER_SPLIT, s)) return -1;
        if (lstm ? launch_lstm_proj(s, S, I, in, out, m->iWp[l].as<unsigned>(), m->ibs[l].as<float>(), m->sWp[l].as<unsigned>(), m->lp[l].as<float>(),
                                    mp.md, backward, mp.lanes1, lg.gru1_nwg)
                 : launch_gru_proj(s, S, in, out, resid, m->iWp[l].as<unsigned>(), m->ibs[l].as<float>(), m->sWp[l].as<unsigned>(), m->sW2p[l].as<unsigned>(),
                                   mp.md, backward, mp.lanes1, lg.gru1_nwg, mp.lanes, lg.gru_nwg, lg.gru_two)) return -1;
    } else {
        if (e->d_xaff.ensure((size_t)c.ncb * gates * S * 16 * 4)) return -1;      /* (a no-op: run_pipeline has sized it for every layer that gets here) */
        if (launch_affine(s, I, in, e->d_xaff.as<float>(), m->iW[l].as<float>(), m->iWp[l].as<unsigned>(), m->ib[l].as<float>(), m->ibs[l].as<float>(), c.ncb, gates * S / 16, f32)) return -1;
        if (c.pf.mark(Marks::LAYER_SPLIT, s)) return -1;
        if (lstm ? launch_lstm(s, S, e->d_xaff.as<float>(), out, m->sWp[l].as<unsigned>(), m->lp[l].as<float>(), mp.md, backward, mp.lanes, lg.gru_nwg)
                 : launch_gru(s, S, e->d_xaff.as<float>(), out, resid, m->sW[l].as<float>(), m->sW2[l].as<float>(), m->sWp[l].as<unsigned>(), m->sW2p[l].as<unsigned>(),
                              mp.md, backward, lg.ntile, mp.lanes, lg.gru_nwg, f32)) return -1;
    }
    if (c.pf.mark(Marks::LAYER_END, s)) return -1;
    c.pf.span(F_AFFINE, Marks::LAYER_BEGIN, Marks::LAYER_SPLIT);
    c.pf.span(F_GRU, Marks::LAYER_SPLIT, Marks::LAYER_END);
    if (c.pf.on) {
        scrappie_hip_timing &tm = sl.timing;
        const double af = 2.0 * I * gates * S * 16.0 * (double)c.ncb, gf = 2.0 * gates * S * S * 16.0 * (double)c.ncb;
        tm.n_affine_launches++; tm.n_gru_launches++; tm.affine_flops += af; tm.gru_flops += gf;
        if (one_kernel) { tm.n_fused_launches++; tm.fused_flops += af + gf; }
    }
    if (one_kernel) c.pf.span(F_FUSED, Marks::LAYER_SPLIT, Marks::LAYER_END);
    return 0;
}

/* Stage 2: the recurrent layers.  *top: which of c.abuf holds the trunk's output. */
static int stage_trunk(Slot &sl, Model *m, GroupRun &c, int *top) {
    const hipStream_t s = c.s;
    const int S = m->S, F = m->F;
    float **abuf = c.abuf; *top = 0;
    if (m->arch == 2 || m->arch == 3) {
        /* raw_r94 (networks.c:196-247; GRU) and events (networks.c:159-181; LSTM): per level, forward and backward layer on the same input,
         * joined by feedforward2_tanh, which writes over the input */
        for (int lvl = 0; lvl < 2 && lvl < c.trunk_upto; lvl++) {
            for (int dir = 0; dir < 2; dir++) if (recurrent_layer(sl, m, c, 2 * lvl + dir, lvl == 0 ? F : S, abuf[0], abuf[1 + dir], dir)) return -1;
            if (c.pf.mark(Marks::LAYER_BEGIN, s)) return -1;
            if (launch_affine2(s, S, abuf[1], abuf[2], abuf[0], m->ff2W[lvl][0].as<unsigned>(), m->ff2W[lvl][1].as<unsigned>(), m->ff2b[lvl].as<float>(), c.ncb, S / 16)) return -1;
            if (c.pf.mark(Marks::LAYER_SPLIT, s)) return -1;
            c.pf.span(F_AFFINE, Marks::LAYER_BEGIN, Marks::LAYER_SPLIT);
            if (c.pf.on) sl.timing.affine_flops += 2.0 * 2 * S * S * 16.0 * (double)c.ncb;
        }
    } else {
        /* rgrgr / rnnrf stacks: five layers in alternating directions, ping-pong between two buffers */
        for (int l = 0; l < 5 && l < c.trunk_upto; l++, *top ^= 1)
            if (recurrent_layer(sl, m, c, l, l == 0 ? F : S, abuf[*top], abuf[*top ^ 1], (l % 2 == 0) ? 1 : 0)) return -1;
    }
    HIPCHK(hipGetLastError());
    c.stamp("layers enqueued at");
    return 0;
}

/* Caller-supplied data in place of a stage's output (scrappie_hip_set_trunk_input, scrappie_hip_set_decoder_input): their image in the group's chunk
 * layout is built once per launch-group shape and re-used.  grow() sizes the image, launch(grid, offsets) enqueues the kernel that builds it. */
template <class Grow, class Launch>
static int inject_alt(const Slot &sl, GroupRun &c, AltInput &alt, uint64_t seed, Grow grow, Launch launch) {
    const LaunchGroup &lg = sl.lg;
    std::vector<unsigned long long> aoff(lg.npad, ~0ull);
    uint64_t key = 1469598103934665603ull ^ seed;
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o >= 0 && lg.rT[i] > 0) aoff[i] = alt.off[(size_t)o % alt.off.size()];
        key = (key ^ (uint64_t)(aoff[i] + 0x9e3779b97f4a7c15ull * (uint64_t)(lg.rT[i] + 1))) * 1099511628211ull;
    }
    if (alt.valid && key == alt.key) return 0;
    if (grow() || alt.d_off.ensure(lg.npad * 8)) return -1;
    HIPCHK(hipMemcpyAsync(alt.d_off.p, aoff.data(), lg.npad * 8, hipMemcpyHostToDevice, c.s));
    HIPCHK(sh_stream_wait(c.s));          /* aoff is a local */
    launch(dim3((unsigned)lg.ntile, (unsigned)std::min(longest_tile(lg), 1024)), alt.d_off.as<unsigned long long>());
    alt.key = key; alt.valid = true;
    return 0;
}

/* Stage 3, transducer models: output layer (S1) + Viterbi decoder, the traceback walk where it is a kernel of its own.  *stopped: the caller wanted
 * the posterior and nothing behind it. */
static int stage_decode_transducer(Slot &sl, Model *m, GroupRun &c, const float *top, bool fused, bool *stopped) {
    scrappie_hip_engine *e = c.e;
    LaunchGroup &lg = sl.lg; const MetaPtrs &mp = c.mp;
    const hipStream_t s = c.s; const scrappie_hip_params *p = c.p;
    const int S = m->S, mtiles = m->ff_mtiles;
    const long long ncb = c.ncb;
    if (e->d_sums.ensure((size_t)ncb * 16 * 4)) return -1;
    if (c.pf.mark(Marks::S1_BEGIN, s)) return -1;
    if (!fused && launch_ff(s, S, top, e->d_E.as<float>(), e->d_sums.as<float>(), m->ffWp.as<unsigned>(), m->ffbs.as<float>(),
                            ncb, mtiles, m->NS, p->tempW / p->tempb, p->tempb, e->ncu)) return -1;
    if (c.pf.mark(Marks::S1_END, s)) return -1;
    c.pf.span(F_FF, Marks::S1_BEGIN, Marks::S1_END);
    if (c.pf.on) sl.timing.ff_flops += 2.0 * S * m->NS * 16.0 * (double)ncb;
    const float *E_use = e->d_E.as<float>(), *sums_use = e->d_sums.as<float>();
    if (e->alt_prob) {
        /* measurement / test hook: the decoder (and scrappie_hip_posterior) see the caller's probabilities instead */
        if (inject_alt(sl, c, e->alt_prob, (uint64_t)lg.model,
                       [&] { return e->d_Ealt.ensure((size_t)ncb * mtiles * 256 * 4) || e->d_sums_alt.ensure((size_t)ncb * 16 * 4); },
                       [&](dim3 grid, const unsigned long long *off) {
                           hipLaunchKernelGGL(k_inject_prob, grid, dim3(256), 0, s, e->alt_prob.data, off, mp.md, m->NS, mtiles, e->d_Ealt.as<float>(), e->d_sums_alt.as<float>());
                       })) return -1;
        E_use = e->d_Ealt.as<float>(); sums_use = e->d_sums_alt.as<float>();
    }
    if (c.ro) { c.ro->E = E_use; c.ro->sums = sums_use; }
    if (c.stop == STOP_POST) { HIPCHK(hipGetLastError()); *stopped = true; return 0; }
    const int NH = m->NS - 1, NQ = NH / 4;
    if (e->d_tb.ensure((size_t)ncb * NQ * 16 * 4) || e->d_tbend.ensure((size_t)ncb * 16 * 4) || e->d_fstate.ensure(lg.npad * 4)) return -1;
    if (c.hp_on && sl.d_hp.ensure((size_t)std::max<long long>(lg.nhp, 1) * 5 * 4)) return -1;
    ShVitArgs va;
    va.E = E_use; va.sums = sums_use;
    va.strideT = (long long)mtiles * 256; va.strideQ = 64; va.strideB = 4;
    va.want_log = 1; va.min_prob = p->min_prob;
    va.stay_pen = p->stay_pen; va.skip_pen = p->skip_pen; va.local_pen = p->local_pen; va.use_slip = p->use_slip;
    va.tb = e->d_tb.as<unsigned>(); va.tb_end = e->d_tbend.as<int>();
    va.final_state = e->d_fstate.as<int>(); va.final_score = sl.d_fscore.as<float>();
    va.hp_side = c.hp_on ? sl.d_hp.as<float>() : nullptr; va.hp_off = mp.hp_off;
    va.dbg = nullptr;
    va.dump_final = e->dbg_dump_final ? 1 : 0;
    static StampBuf vst;      /* SH_VIT_STAMP: cycle stamps of every decoder launch on stderr (tuning aid) */
    if (tun().vit_stamp) va.dbg = vst.dev(4096 * 16 * 8);
    /* more tiles than CUs: tiles are cut between workgroups, which hand their state over through HBM (sh_sched.h): the two-team kernel's
     * workgroups walk a lane of segments each, the other two kernels own one piece of a tile per workgroup */
    if (e->d_vstate.ensure(std::max<size_t>(lg.ntile, 1) * ((size_t)NH * 16 + 32) * 4) || e->d_vflag.ensure(std::max<size_t>(lg.ntile, 1) * 4)) return -1;
    HIPCHK(hipMemsetAsync(e->d_vflag.p, 0, std::max<size_t>(lg.ntile, 1) * 4, s));
    va.seg = mp.vseg; va.lane_off = nullptr;
    const bool teams = fused && !p->use_slip && !(tun().fv_single || e->dbg_fv_single);
    if (teams) { va.seg = mp.vlseg; va.lane_off = mp.vloff; }
    const int vit_nwg = teams ? lg.vit_lane_nwg : lg.vit_nwg;
    lg.vit_launched = teams ? lg.vit_lane_nseg : lg.vit_nwg; lg.vit_launched_wg = vit_nwg;
    va.vstate = e->d_vstate.as<float>(); va.flag = e->d_vflag.as<unsigned>(); va.err = sl.d_gflag.as<unsigned>() + lg.ntile;
    /* the other slot's traceback walk (on the copy stream) reads the buffers this decode overwrites */
    if (e->ev_ok && e->other(sl).pending) HIPCHK(hipStreamWaitEvent(s, e->other(sl).done, 0));
    if (fused) {
        ShFfArgs fa;
        fa.in = top; fa.wpiece = m->ffWp.as<unsigned>(); fa.bfrag = m->ffbs.as<float>();
        fa.in_div = p->tempW / p->tempb; fa.out_div = p->tempb;
        fa.no_clamp = (m->ff_no_clamp && !e->alt_trunk) ? 1 : 0;      /* (the trunk-input hook feeds activations that need not be gate outputs) */
        va.E = nullptr; va.sums = nullptr;
        if (launch_ff_viterbi(s, fa, va, mp.md, (size_t)vit_nwg, !teams)) return -1;
    } else if (launch_viterbi(s, NH, va, mp.md, (size_t)vit_nwg)) return -1;
    if (va.dbg) vst.dump_on(0, s, (size_t)std::max(vit_nwg, 1) * 16 * 8, [&](const unsigned long long *h) {
        const int nwv = teams ? 12 : 8;       /* the two-team kernel stamps twelve waves (8-11: the S1 team) */
        for (int w = 0; w < nwv; w++) {
            const unsigned long long *d = &h[((size_t)(vit_nwg / 2) * nwv + w) * 8];
            fprintf(stderr, "vit stamp wave %d: phaseB %.0f bar %.0f phaseC %.0f bar %.0f cycles/block", w, d[0] / (double)d[4], d[1] / (double)d[4], d[2] / (double)d[4], d[3] / (double)d[4]);
            /* the two-team kernel: what a segment costs outside the block loop, from its first instruction to the barrier that opens the loop */
            if (teams && d[6]) fprintf(stderr, "; %llu blocks in %llu segments, prologue %.0f cycles/segment", d[4], d[6], d[5] / (double)d[6]);
            fprintf(stderr, "\n");
        }
    });
    if (c.pf.mark(Marks::DECODE_END, s)) return -1;
    c.pf.span(F_DECODE, Marks::S1_END, Marks::DECODE_END);
    c.stamp("decoder enqueued at");
    /* the traceback walk is a chain of dependent loads per read (latency, hardly any CUs): it runs on the
     * copy stream, under the next group's first kernels, in front of the result copies */
    c.walk_on_cs = e->ev_ok;
    if (c.walk_on_cs) { HIPCHK(hipEventRecord(sl.kdone, s)); HIPCHK(hipStreamWaitEvent(e->cstream, sl.kdone, 0)); }
    /* walk back + stitching + result transfer as one kernel behind the decoder (k_walk_stitch_out) whenever the stitching is the device's and the copy
     * stream exists; three kernels otherwise (and for the flip-flop models, whose walk back is k_crf's) */
    c.fold_tail = c.walk_on_cs && !tun().split_tail && !tun().host_stitch;
    if (!c.fold_tail) {
        hipStream_t bs = c.walk_on_cs ? e->cstream : s;
        if (c.pf.mark(Marks::WALK_BEGIN, bs)) return -1;
        hipLaunchKernelGGL(k_backtrace, dim3((unsigned)((lg.npad + 63) / 64)), dim3(64), 0, bs, e->d_tb.as<unsigned>(), e->d_tbend.as<int>(),
                           e->d_fstate.as<int>(), mp.md, mp.seq_off, sl.d_seq.as<int>(), (int)lg.npad, NQ, SH_SEQ_STRIDE);
        if (c.pf.mark(Marks::WALK_END, bs)) return -1;
        c.pf.span(F_BACKTRACE, Marks::WALK_BEGIN, Marks::WALK_END);
    }
    return 0;
}

/* Stage 3, flip-flop (CRF) models: output layer + k_crf (decoder and walk back in one) */
static int stage_decode_crf(Slot &sl, Model *m, GroupRun &c, const float *top, bool *stopped) {
    scrappie_hip_engine *e = c.e;
    LaunchGroup &lg = sl.lg; const MetaPtrs &mp = c.mp;
    const hipStream_t s = c.s;
    const int S = m->S, mtiles = m->ff_mtiles;
    const long long ncb = c.ncb;
    if (c.pf.mark(Marks::S1_BEGIN, s)) return -1;
    if (launch_affine(s, S, top, e->d_E.as<float>(), m->ffW.as<float>(), m->ffWp.as<unsigned>(), m->ffb.as<float>(), m->ffbs.as<float>(), ncb, mtiles)) return -1;
    if (c.pf.mark(Marks::S1_END, s)) return -1;
    c.pf.span(F_FF, Marks::S1_BEGIN, Marks::S1_END);
    if (c.pf.on) sl.timing.ff_flops += 2.0 * S * m->NS * 16.0 * (double)ncb;
    if (e->d_tb.ensure((size_t)ncb * 16 * 8)) return -1;         /* one byte per state (8 per read) and block */
    /* d_tb is shared by the two slots: a transducer group in the other slot may still be walking it
     * (k_backtrace on the copy stream) */
    if (e->ev_ok && e->other(sl).pending) HIPCHK(hipStreamWaitEvent(s, e->other(sl).done, 0));
    /* (only the posterior surface and k_crf_post look at the normalised transitions afterwards: the plain basecall path does not write them back) */
    const bool probs = lg.post.on && c.stop == STOP_NONE;
    hipLaunchKernelGGL((c.ro || c.stop == STOP_POST || probs) ? k_crf<true> : k_crf<false>, dim3((unsigned)(lg.npad / 16)), dim3(128), 0, s, e->d_E.as<float>(), mp.md,
                       e->d_tb.as<unsigned char>(), mp.seq_off, sl.d_seq.as<int>(), sl.d_fscore.as<float>(), (int)lg.npad, SH_SEQ_STRIDE);
    if (c.pf.mark(Marks::DECODE_END, s)) return -1;
    c.pf.span(F_DECODE, Marks::S1_END, Marks::DECODE_END);
    if (c.ro) { c.ro->E = e->d_E.as<float>(); c.ro->sums = nullptr; }
    if (c.stop == STOP_POST) { HIPCHK(hipGetLastError()); *stopped = true; }
    /* base probabilities: on the main stream, before the next group's output layer can overwrite d_E (the engine's, not the slot's) */
    if (probs && crf_post_enqueue(sl, c)) return -1;
    return 0;
}

/* Stage 4: walk back and stitching where they are the device's, results -> pinned host buffers on the copy stream, the slot's done event.  The
 * per-slot device buffers are not touched again before this slot is collected, so the next group's kernels need not wait for PCIe. */
static int stage_tail(Slot &sl, Model *m, GroupRun &c) {
    scrappie_hip_engine *e = c.e;
    LaunchGroup &lg = sl.lg; const MetaPtrs &mp = c.mp;
    const hipStream_t s = c.s, cs = c.cs;
    if (sl.h_score.ensure(lg.npad * 4)) return -1;
    if (sl.h_err.ensure(4) || sl.h_bad.ensure(lg.npad * 4)) return -1;
    if (c.pf.mark(Marks::MAIN_END, s)) return -1;
    c.pf.span(F_TOTAL, Marks::MAIN_BEGIN, Marks::MAIN_END);        /* (the convolution ran on the prologue stream, under the previous group) */
    if (e->ev_ok && !c.walk_on_cs) { HIPCHK(hipEventRecord(sl.kdone, s)); HIPCHK(hipStreamWaitEvent(cs, sl.kdone, 0)); }
    /* D2 + D3 on the device (k_stitch, behind the traceback walk on the copy stream): bases, not paths, go to the host */
    lg.dev_stitch = !tun().host_stitch;
    lg.dev_pos = lg.dev_stitch && c.p->want_pos != 0 && c.transducer;
    if (lg.dev_stitch) {
        const size_t nseq = (size_t)std::max<long long>(lg.nseq, 1), ncap = (size_t)std::max<long long>(lg.nbases_cap, 1);
        if (sl.d_bases.ensure(ncap) || sl.d_blen.ensure(lg.npad * 4) || sl.d_redo.ensure(lg.npad * 4) ||
            sl.h_bases.ensure(ncap) || sl.h_blen.ensure(lg.npad * 4) || sl.h_redo.ensure(lg.npad * 4)) return -1;
        if (lg.dev_pos && (sl.d_pos.ensure(nseq * 4 + 16) || sl.h_pos.ensure(nseq * 4 + 16))) return -1;
        ShStitchArgs sa;
        sa.seq = sl.d_seq.as<int>(); sa.seq_off = mp.seq_off;
        sa.hp = c.hp_on ? sl.d_hp.as<float>() : nullptr; sa.hp_off = mp.hp_off;
        sa.pos = lg.dev_pos ? sl.d_pos.as<int>() : nullptr;
        sa.bases = sl.d_bases.as<char>(); sa.bases_off = mp.bases_off;
        sa.blen = sl.d_blen.as<int>(); sa.redo = sl.d_redo.as<unsigned>();
        sa.npad = (int)lg.npad; sa.nstate = m->NS; sa.crf = c.transducer ? 0 : 1; sa.sstride = SH_SEQ_STRIDE;
        /* results into pinned host memory by the device itself (k_results_out): bases of exactly the called length, the
         * per-read words, the error word; pos[] (rarely wanted) likewise, whole */
        ShResultArgs ra;
        ra.d_bases = sl.d_bases.as<char>(); ra.h_bases = sl.h_bases.as<char>(); ra.bases_off = mp.bases_off;
        ra.d_blen = sl.d_blen.as<int>(); ra.h_blen = sl.h_blen.as<int>();
        ra.d_redo = sl.d_redo.as<unsigned>(); ra.h_redo = sl.h_redo.as<unsigned>();
        ra.d_score = sl.d_fscore.as<float>(); ra.h_score = sl.h_score.as<float>();
        ra.d_bad = sl.d_bad.as<unsigned>(); ra.h_bad = sl.h_bad.as<unsigned>();
        ra.d_err = sl.d_gflag.as<unsigned>() + lg.ntile; ra.h_err = sl.h_err.as<unsigned>();
        ra.npad = (int)lg.npad;
        if (c.pf.mark(Marks::STITCH_BEGIN, cs)) return -1;
        const bool dwell = lg.dw.on && c.transducer;      /* events with the dwell correction: the stitching's other form (sh_dwell.h) */
        if (c.fold_tail) {
            ShWalkArgs wa;
            wa.tb = e->d_tb.as<unsigned>(); wa.tb_end = e->d_tbend.as<int>(); wa.final_state = e->d_fstate.as<int>();
            wa.seq_off = mp.seq_off; wa.seq = sl.d_seq.as<int>(); wa.NQ = (m->NS - 1) / 4;
            if (dwell) hipLaunchKernelGGL(k_walk_dwell_out, dim3((unsigned)((lg.npad + 63) / 64)), dim3(64), 0, cs, wa, sa, mp.dw, ra, mp.md);
            else hipLaunchKernelGGL(k_walk_stitch_out, dim3((unsigned)((lg.npad + 63) / 64)), dim3(64), 0, cs, wa, sa, ra, mp.md);
        } else if (dwell)
            hipLaunchKernelGGL(k_stitch_dwell, dim3((unsigned)((lg.npad + 63) / 64)), dim3(64), 0, cs, sa, mp.dw);
        else
            hipLaunchKernelGGL(k_stitch, dim3((unsigned)((lg.npad + 63) / 64)), dim3(64), 0, cs, sa, mp.md);
        if (c.pf.mark(Marks::STITCH_END, cs)) return -1;
        c.pf.span(F_STITCH, Marks::STITCH_BEGIN, Marks::STITCH_END);
        if (e->ev_ok) HIPCHK(hipEventRecord(sl.hdone, cs));
        c.stamp("stitch enqueued at");
        if (!c.fold_tail) hipLaunchKernelGGL(k_results_out, dim3((unsigned)((lg.npad + 3) / 4)), dim3(256), 0, cs, ra);
        if (lg.dev_pos) {
            const long long n16 = (lg.nseq * 4 + 15) / 16;
            hipLaunchKernelGGL(k_upload_words, dim3((unsigned)std::min<long long>((n16 + 255) / 256, 256)), dim3(256), 0, cs, (const u32x4 *)sl.d_pos.p, sl.h_pos.as<u32x4>(), n16);
        }
    } else {      /* paths (+ side rows) and the per-read words by copies: the host stitches */
        if (sl.h_seq.ensure((size_t)std::max<long long>(lg.nseq, 1) * 4)) return -1;
        if (c.hp_on && sl.h_hp.ensure((size_t)std::max<long long>(lg.nhp, 1) * 5 * 4)) return -1;
        HIPCHK(hipMemcpyAsync(sl.h_seq.p, sl.d_seq.p, (size_t)lg.nseq * 4, hipMemcpyDeviceToHost, cs));
        if (c.hp_on) HIPCHK(hipMemcpyAsync(sl.h_hp.p, sl.d_hp.p, (size_t)lg.nhp * 5 * 4, hipMemcpyDeviceToHost, cs));
        HIPCHK(hipMemcpyAsync(sl.h_score.p, sl.d_fscore.p, lg.npad * 4, hipMemcpyDeviceToHost, cs));
        HIPCHK(hipMemcpyAsync(sl.h_err.p, sl.d_gflag.as<unsigned>() + lg.ntile, 4, hipMemcpyDeviceToHost, cs));
        HIPCHK(hipMemcpyAsync(sl.h_bad.p, sl.d_bad.p, lg.npad * 4, hipMemcpyDeviceToHost, cs));
    }
    /* the base probabilities behind the slot's results, in front of its done event: the next group's kernels do not wait for PCIe */
    if (lg.post.on && crf_post_download(sl, c)) return -1;
    HIPCHK(hipGetLastError());
    c.stamp("copies enqueued at");
    if (e->ev_ok) HIPCHK(hipEventRecord(sl.done, cs));
    return 0;
}

static int run_pipeline(scrappie_hip_engine *e, Model *m, const float *d_signal, const uint64_t *offsets,
                        const uint32_t *lengths, size_t n, const scrappie_hip_params *p, StopAt stop,
                        int trunk_upto, RunOut *ro, const DwellJob *dw = nullptr, const PostJob *pj = nullptr) {
    (void)hipSetDevice(e->device);
    if (n == 0) return set_err("empty batch");
    GroupRun c;
    c.e = e; c.d_signal = d_signal; c.offsets = offsets; c.p = p; c.stop = stop; c.trunk_upto = trunk_upto; c.ro = ro; c.dw = dw; c.pj = pj;
    c.transducer = (m->arch != 1);
    c.hp_on = c.transducer && p->homopolymer == HOMOPOLYMER_MEAN && stop == STOP_NONE;
    c.s = e->stream; c.ps = e->ev_ok ? e->pstream : e->stream; c.cs = e->ev_ok ? e->cstream : e->stream;
    Slot *slp = nullptr; bool empty = false;
    if (begin_group(e, m, lengths, n, c, &slp, &empty)) return -1;
    if (empty) return 0;
    Slot &sl = *slp;
    LaunchGroup &lg = sl.lg;
    const long long ncb = c.ncb = lg.ncb;
    const int S = m->S, F = m->F;
    c.act_bytes = (size_t)ncb * std::max(S, F) * 16 * 4;
    if (e->d_act[1].ensure(c.act_bytes)) return -1;
    /* gate inputs in HBM: only where projection and recurrence are separate kernels */
    bool any_f32 = false;
    for (bool b : m->layer_f32) any_f32 |= b;
    const bool need_xaff = m->arch == 3 || !gru_proj_ok(F, S) || tun().gru_separate || any_f32;
    if (need_xaff && e->d_xaff.ensure((size_t)ncb * (m->arch == 3 ? 4 : 3) * S * 16 * 4)) return -1;
    if ((m->arch == 2 || m->arch == 3) && e->d_act[2].ensure(c.act_bytes)) return -1;
    c.pf.sl = &sl; c.pf.on = e->profiling && e->ev_ok;
    if (c.pf.on) { memset(&sl.timing, 0, sizeof sl.timing); sl.nev = 0; sl.spans.clear(); }
    if (stage_prologue(sl, m, c)) return -1;
    if (lg.post.on && e->ev_ok && crf_post_mark(sl, 0, c.s)) return -1;      /* (PEV_MAIN: the main stream's part of the group starts here) */
    int cur = 0;
    if (stage_trunk(sl, m, c, &cur)) return -1;
    if (ro) { ro->act = c.abuf[cur]; ro->act_units = (trunk_upto == 0) ? F : S; }
    lg.model = (int)(std::find(e->models.begin(), e->models.end(), m) - e->models.begin());
    if (stop == STOP_TRUNK) { lg.valid = true; return 0; }
    /* what the output layer reads: the trunk's output -- or, under scrappie_hip_set_trunk_input, the caller's
     * activations (the network above has run in full either way) */
    const float *top = c.abuf[cur];
    if (e->alt_trunk) {
        if (inject_alt(sl, c, e->alt_trunk, (uint64_t)lg.model ^ ((uint64_t)S << 32),
                       [&] { return e->d_act_alt.ensure((size_t)ncb * S * 16 * 4); },
                       [&](dim3 grid, const unsigned long long *off) {
                           hipLaunchKernelGGL(k_inject_trunk, grid, dim3(256), 0, c.s, e->alt_trunk.data, off, c.mp.md, S, e->d_act_alt.as<float>());
                       })) return -1;
        top = e->d_act_alt.as<float>();
    }
    const bool fused = c.transducer && stop == STOP_NONE && decoder_fused(e, m);
    if (!fused && e->d_E.ensure((size_t)ncb * m->ff_mtiles * 256 * 4)) return -1;
    if (sl.d_seq.ensure((size_t)std::max<long long>(lg.nseq, 1) * 4) || sl.d_fscore.ensure(lg.npad * 4)) return -1;
    bool stopped = false;
    if (c.transducer ? stage_decode_transducer(sl, m, c, top, fused, &stopped) : stage_decode_crf(sl, m, c, top, &stopped)) return -1;
    if (stopped) { lg.valid = true; return 0; }
    HIPCHK(hipGetLastError());
    if (stage_tail(sl, m, c)) return -1;
    lg.valid = true;
    lg.d_signal = d_signal; lg.in_off.assign(offsets, offsets + n); lg.in_len.assign(lengths, lengths + n); lg.params = *p;
    mark_pending(e, sl);
    return 0;
}

/* A launch group from host signals, for the callers that want something other than base calls (posterior_batch, map_group; under mu): the reads' windows
 * laid end to end into the first slot's h_sig / d_signal (nothing else is in flight under mu), uploaded and waited for (the group's prologue runs on
 * another stream: the signals must be there before it is enqueued), run_pipeline to `stop`, and the group's range flags back in bad[npad] (tiled order,
 * as e->current().lg).  The reads are long enough for the model.  ms: += the time from the upload to the flags' arrival. */
static int run_staged(scrappie_hip_engine *e, Model *m, const std::vector<const raw_table *> &win, const scrappie_hip_params *p, StopAt stop,
                      int trunk_upto, RunOut *ro, std::vector<unsigned> &bad, double *ms = nullptr) {
    const size_t cnt = win.size();
    std::vector<uint64_t> off(cnt);
    std::vector<uint32_t> len(cnt);
    size_t total = 0;
    for (size_t k = 0; k < cnt; k++) {
        const size_t nf = win[k]->end - win[k]->start;
        off[k] = total; len[k] = (uint32_t)(m->arch == 3 ? nf / (size_t)m->nfeat : nf);      /* events: raw holds [nevent][12] features */
        total += nf;
    }
    Slot &st = e->slots[0];
    if (st.h_sig.ensure(total * 4) || st.d_signal.ensure(total * 4)) return -1;
    float *hs = st.h_sig.as<float>();
    for (size_t k = 0; k < cnt; k++) memcpy(hs + off[k], win[k]->raw + win[k]->start, (win[k]->end - win[k]->start) * 4);
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpyAsync(st.d_signal.p, hs, total * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(sh_stream_wait(e->stream));
    if (run_pipeline(e, m, st.d_signal.as<float>(), off.data(), len.data(), cnt, p, stop, trunk_upto, ro)) return -1;
    const Slot &sl = e->current();
    bad.assign(sl.lg.npad, 0);
    HIPCHK(hipMemcpyAsync(bad.data(), sl.d_bad.p, sl.lg.npad * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(sh_stream_wait(e->stream));
    if (ms) *ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
