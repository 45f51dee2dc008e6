/* sh_eng_surface.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * the reference's per-read functions: posterior / trunk on an explicit engine, the process-default engine, decode_transducer, decode_crf.
 * Each family has ONE implementation, a batch function (posterior_batch, decode_batch, crf_batch): the queue (sh_coalesce.h) hands it the calls that were
 * waiting, a call by itself -- explicit engine, or SCRAPPIE_HIP_COALESCE=0 -- hands it a batch of one.  The batch functions take the engine's lock and stage
 * through buffers the engine owns, so callers that come in without the queue are kept apart by that lock alone. */

/* ------------------------------------------------------------------ */
/* the network: posterior / trunk of the reads of one launch group      */
/* ------------------------------------------------------------------ */
/* Posteriors of several reads in one launch group: what the queue below assembles from the calls of several host threads, and -- as a batch of one --
 * a call on an explicit engine or with the queue off.  Every request gets its own host matrix or its own error text; a read's posterior does not
 * depend on what it was batched with.  The requests of a batch share model, temperatures and stopping point. */
struct PostReq {
    int model = -1;
    raw_table sig{};
    float min_prob = 0.f, tempW = 1.f, tempb = 1.f;
    bool want_log = true;
    StopAt stop = STOP_POST;         /* STOP_TRUNK: the activations after layer `upto` instead of the posterior (scrappie_hip_trunk) */
    int upto = 5;
    scrappie_matrix out = nullptr;
    size_t nr = 0, nc = 0;           /* shape of the matrix to make */
    const float *src = nullptr;      /* the matrix's bytes in the batch's pinned buffer: the caller makes the matrix and copies them itself (all callers at once) */
    size_t nbytes = 0;
    std::atomic<int> *users = nullptr;
    int phase = 0;                   /* sh_coalesce.h: 0 queued ... 3 done */
    char err[256] = "";
};
static void post_fail(PostReq *r, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r->err, sizeof r->err, fmt, ap);
    va_end(ap);
}
static void posterior_batch(scrappie_hip_engine *e, std::vector<PostReq *> &reqs) {
    if (reqs.empty()) return;
    Model *m = get_model(e, reqs[0]->model);
    if (!m) { for (PostReq *r : reqs) post_fail(r, "%s", g_err); return; }
    const bool trunk = reqs[0]->stop == STOP_TRUNK;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    PostStage *stage = &e->post_stage[e->post_turn++ & 1];
    std::vector<PostReq *> live;
    std::vector<const raw_table *> win;
    for (PostReq *r : reqs) {
        const raw_table &sg = r->sig;
        if (sg.n == 0 || !sg.raw || sg.end <= sg.start) { post_fail(r, "empty read"); continue; }
        const size_t nf = sg.end - sg.start, ns = m->arch == 3 ? nf / (size_t)m->nfeat : nf;      /* events: raw holds [nevent][12] features */
        if (ns < m->min_samples) {
            if (trunk) post_fail(r, "read too short");
            else post_fail(r, "read of %zu samples is below the model minimum %zu", ns, m->min_samples);
            continue;
        }
        live.push_back(r); win.push_back(&r->sig);
    }
    if (live.empty()) return;
    scrappie_hip_params p = scrappie_hip_default_params();
    p.tempW = live[0]->tempW; p.tempb = live[0]->tempb;
    RunOut ro;
    std::vector<unsigned> bad;
    if (run_staged(e, m, win, &p, live[0]->stop, live[0]->upto, &ro, bad)) { for (PostReq *r : live) post_fail(r, "%s", g_err); return; }
    /* what is gathered: the posterior where S1 left it (finalised here for the transducers; the CRF's transitions are final), or the trunk's activations */
    const float *src = trunk ? ro.act : ro.E;
    const int nr = trunk ? ro.act_units : m->NS, nchunk = trunk ? ro.act_units / 16 : m->ff_mtiles;
    const bool tr = !trunk && m->arch != 1;
    const LaunchGroup &lg = e->current().lg;
    /* one staging buffer for the whole group, one synchronisation */
    std::vector<size_t> toff(lg.npad, 0);
    size_t tbytes = 0;
    const size_t mstride = (size_t)((nr + 3) / 4) * 4;      /* scrappie_matrix.c:11-42: rows padded to whole vectors */
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0) continue;
        PostReq *r = live[(size_t)o];
        if (bad[i]) { post_fail(r, "the read holds values outside the supported range (|activation| >= %g after the first layer, or non-finite): is the signal trimmed and med/MAD-normalised?", (double)SH_ACT_LIMIT); continue; }
        /* (the matrix itself -- 3.3 MB to allocate and clear for a read of 4000 samples -- is made by the caller, beside all the others) */
        r->nr = (size_t)nr; r->nc = lg.rT[i];
        toff[i] = tbytes; tbytes += (size_t)lg.rT[i] * mstride * 4;
    }
    DBuf &tmp = stage->d;            /* (grow-only, kept between launch groups) */
    bool ok = tbytes == 0 || tmp.ensure(tbytes) == 0;
    ok = ok && (tbytes == 0 || hipMemsetAsync(tmp.p, 0, tbytes, e->stream) == hipSuccess);
    /* the buffer's last batch has been copied out by its callers (two buffers in turn: nearly always long ago) */
    while (stage->users.load(std::memory_order_acquire) > 0) std::this_thread::yield();
    ok = ok && (tbytes == 0 || stage->h.ensure(tbytes) == 0);
    for (size_t i = 0; ok && i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0 || live[(size_t)o]->nc == 0) continue;
        PostReq *r = live[(size_t)o];
        const int T = lg.rT[i];
        const long long tot = (long long)T * nr;
        float *dst = (float *)((char *)tmp.p + toff[i]);
        hipLaunchKernelGGL(k_gather_read, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, e->stream, src, tr ? ro.sums : nullptr, lg.tile_boff[i >> 4], (int)(i & 15), T, nr,
                           nchunk, (int)mstride, tr ? 1 : 0, tr && r->want_log ? 1 : 0, tr ? r->min_prob : 0.f, dst);
    }
    /* one copy into pinned memory at the link's rate; the callers take their matrices out of it themselves, all at once */
    ok = ok && (tbytes == 0 || hipMemcpyAsync(stage->h.p, tmp.p, tbytes, hipMemcpyDeviceToHost, e->stream) == hipSuccess);
    ok = ok && sh_stream_wait(e->stream) == hipSuccess;
    if (!ok) {
        set_err("gather failed: %s", hipGetErrorString(hipGetLastError()));
        for (PostReq *r : live) if (r->nc) { r->nc = 0; post_fail(r, "%s", g_err); }
        return;
    }
    int nuse = 0;
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0 || live[(size_t)o]->nc == 0) continue;
        PostReq *r = live[(size_t)o];
        r->src = (const float *)((const char *)stage->h.p + toff[i]);
        r->nbytes = (size_t)lg.rT[i] * mstride * 4;
        r->users = &stage->users;
        nuse++;
    }
    stage->users.store(nuse, std::memory_order_release);
}

/* the caller's half of a batch, on its own thread with the engine's lock released: its matrix, made here and filled from the batch's pinned buffer
 * (3.3 MB to allocate, clear and copy for a read of 4000 samples: the callers of a batch do it all at once), or its error text */
static scrappie_matrix post_result(PostReq &r) {
    if (r.src) {
        r.out = make_scrappie_matrix(r.nr, r.nc);
        if (r.out) memcpy(r.out->data.f, r.src, r.nbytes);
        else post_fail(&r, "out of host memory");
        r.users->fetch_sub(1, std::memory_order_release);
    }
    if (!r.out && r.err[0]) set_err("%s", r.err);
    return r.out;
}
/* a call by itself (explicit engine, or the queue off): a batch of one, run at once; calls are serialised on the engine */
static scrappie_matrix posterior_alone(scrappie_hip_engine *e, PostReq &r) {
    std::vector<PostReq *> one{&r};
    posterior_batch(e, one);
    return post_result(r);
}

extern "C" scrappie_matrix scrappie_hip_posterior(scrappie_hip_engine *e, int model, const raw_table signal, float min_prob,
                                                  float tempW, float tempb, bool return_log) {
    PostReq r;
    r.model = model; r.sig = signal; r.min_prob = min_prob; r.tempW = tempW; r.tempb = tempb; r.want_log = return_log;
    return posterior_alone(e, r);
}

extern "C" scrappie_matrix scrappie_hip_trunk(scrappie_hip_engine *e, int model, const raw_table signal, int upto) {
    PostReq r;
    r.model = model; r.sig = signal; r.stop = STOP_TRUNK; r.upto = upto;
    return posterior_alone(e, r);
}

/* The reference calls its network functions from an OpenMP loop over reads (scrappie_raw.c:355,387), one read per call.  One read cannot fill the
 * device -- its five recurrent layers are a serial chain of T steps each -- so calls that arrive while the device is busy (or within a short window
 * of the first) are run as ONE launch group: whoever finds no batch running becomes its leader, takes every waiting request for the same model and
 * temperatures, runs them, hands the matrices out and wakes the others.  SCRAPPIE_HIP_COALESCE=0: no queue -- every call runs the batch function
 * with its one request, one read per launch, calls serialised on the engine;
 * SCRAPPIE_HIP_COALESCE_US / _MAX_US: the leader's waiting windows (defaults 500 / 10000 microseconds); the queue itself is sh_coalesce.h. */
/* how many host threads are inside the coalesced functions (either of them), and the most seen lately: a process that calls from ONE thread must not
 * wait for company that cannot come, one that calls from many should */
static ShPresence g_presence;           /* threads inside the per-read functions: how much company a leader waits for (sh_coalesce.h) */
static ShCoalescer<PostReq> g_co;
static bool coalesce_on(char which = 'p') {       /* SCRAPPIE_HIP_COALESCE: 0 neither, p the network calls only, d decode_transducer only; default both */
    static const int on = [] { const char *v = getenv("SCRAPPIE_HIP_COALESCE"); return !v ? 3 : v[0] == '0' ? 0 : v[0] == 'p' ? 1 : v[0] == 'd' ? 2 : 3; }();
    return (on & (which == 'd' ? 2 : 1)) != 0;
}
static scrappie_matrix coalesced_posterior(scrappie_hip_engine *e, int model, const raw_table signal, float min_prob, float tempW, float tempb, bool return_log) {
    constexpr size_t MAX_READS = 4096, MAX_BLOCKS = 200000;          /* per launch group: the posterior is materialised (66 KB per block of 16 reads) */
    ShInside inside(g_presence);
    PostReq r;
    r.model = model; r.sig = signal; r.min_prob = min_prob; r.tempW = tempW; r.tempb = tempb; r.want_log = return_log;
    g_co.run(r, g_presence, MAX_READS, false,
        [&](std::deque<PostReq *> &q, std::vector<PostReq *> &batch) {
            take_compatible(q, batch, MAX_READS, MAX_BLOCKS,
                            [](const PostReq *f, const PostReq *c) { return c->model == f->model && c->tempW == f->tempW && c->tempb == f->tempb; },
                            [](const PostReq *c) { return (c->sig.end > c->sig.start ? c->sig.end - c->sig.start : 0) / 4 + 1; });
        },
        [](std::vector<PostReq *> &) { return true; }, [](PostReq &) {},
        [&](std::vector<PostReq *> &batch) { posterior_batch(e, batch); });
    return post_result(r);
}
/* (tests, tools) launch groups the coalescer has run, reads in them, the largest group */
extern "C" void scrappie_hip_coalescer_stats(unsigned long long out[3]) {
    std::lock_guard<std::mutex> lk(g_co.mu);
    out[0] = g_co.n_batches; out[1] = g_co.n_reads; out[2] = g_co.max_batch;
    if (getenv("SCRAPPIE_HIP_COALESCE_TIMES")) fprintf(stderr, "posterior coalescer: %llu launch groups took %.1f ms in all\n", g_co.n_batches, g_co.service_us / 1e3);
}

/* ------------------------------------------------------------------ */
/* per-read reference surface on the process-default engine             */
/* ------------------------------------------------------------------ */
static scrappie_hip_engine *g_default = nullptr;
static std::mutex g_default_mu;

static scrappie_hip_engine *default_engine() {
    std::lock_guard<std::mutex> lk(g_default_mu);
    if (!g_default) {
        const char *dev = getenv("SCRAPPIE_HIP_DEVICE");
        g_default = scrappie_hip_engine_create(dev ? atoi(dev) : 0);
    }
    return g_default;
}

/* name -> handle on the process-default engine, kept OUTSIDE the engine's own lock: a launch group holds that lock for its whole run, and a caller
 * of the per-read surface that had to take it just to look its model up could not join the queue until the group was over (64 threads then arrive
 * one by one behind every group, and every group holds two reads) */
static std::mutex g_models_mu;
static std::map<std::string, int> g_models;

extern "C" int scrappie_hip_register_model(const char *name, const char *path) {
    scrappie_hip_engine *e = default_engine();
    if (!e || !name) return -1;
    std::lock_guard<std::mutex> lk(g_models_mu);
    const int h = scrappie_hip_load_model(e, name, path);
    if (h >= 0) g_models[name] = h;
    return h;
}

static int default_model(scrappie_hip_engine *e, const char *name) {
    /* find-or-load as one step: the reference's loop calls in from many threads at once, and a second load of the same name would replace -- and
     * free -- the model the first caller is already running */
    std::lock_guard<std::mutex> lk(g_models_mu);
    auto it = g_models.find(name);
    if (it != g_models.end()) return it->second;
    int h = scrappie_hip_find_model(e, name);
    if (h < 0) {
        const char *dir = getenv("SCRAPPIE_MODEL_DIR");
        if (!dir) { set_err("model '%s' is not registered and SCRAPPIE_MODEL_DIR is unset (weights are not compiled in)", name); return -1; }
        std::string path = std::string(dir) + "/" + name + ".scrm";
        h = scrappie_hip_load_model(e, name, path.c_str());
    }
    if (h >= 0) g_models[name] = h;
    return h;
}

static scrappie_matrix named_posterior(const char *name, const raw_table signal, float min_prob, float tempW, float tempb, bool return_log) {
    if (signal.n == 0 || !signal.raw) return nullptr;                 /* networks.c:254-255 */
    scrappie_hip_engine *e = default_engine();
    if (!e) return nullptr;
    const int h = default_model(e, name);
    if (h < 0) return nullptr;
    if (coalesce_on()) return coalesced_posterior(e, h, signal, min_prob, tempW, tempb, return_log);
    return scrappie_hip_posterior(e, h, signal, min_prob, tempW, tempb, return_log);
}

extern "C" scrappie_matrix scrappie_hip_events_posterior(scrappie_hip_engine *e, int model, const float *feature3, size_t nevent,
                                                         float min_prob, float tempW, float tempb, bool return_log) {
    Model *m = get_model(e, model);
    if (!m) return nullptr;
    if (m->arch != 3) { set_err("events_posterior: model '%s' is not an events model", m->name.c_str()); return nullptr; }
    if (!feature3 || nevent == 0) { set_err("events_posterior: empty read"); return nullptr; }
    raw_table rt = {nullptr, nevent * (size_t)m->nfeat, 0, nevent * (size_t)m->nfeat, const_cast<float *>(feature3)};
    return scrappie_hip_posterior(e, model, rt, min_prob, tempW, tempb, return_log);
}

/* networks.c:146: features + window on the host, the network on the device */
extern "C" scrappie_matrix nanonet_posterior(const event_table events, float min_prob, float tempW, float tempb, bool return_log) {
    if (events.n == 0 || !events.event || events.end <= events.start) return nullptr;
    scrappie_hip_engine *e = default_engine();
    if (!e) return nullptr;
    const int model = default_model(e, "nanonet_events");
    if (model < 0) return nullptr;
    const size_t n = events.end - events.start;
    std::vector<float> f3(n * 12);
    if (scrappie_hip_event_features(events, f3.data())) return nullptr;
    if (coalesce_on()) {
        raw_table rt = {nullptr, n * 12, 0, n * 12, f3.data()};
        return coalesced_posterior(e, model, rt, min_prob, tempW, tempb, return_log);
    }
    return scrappie_hip_events_posterior(e, model, f3.data(), n, min_prob, tempW, tempb, return_log);
}

extern "C" scrappie_matrix nanonet_raw_posterior(const raw_table s, float mp, float tw, float tb, bool lg) { return named_posterior("raw_r94", s, mp, tw, tb, lg); }
extern "C" scrappie_matrix nanonet_rgrgr_r94_posterior(const raw_table s, float mp, float tw, float tb, bool lg) { return named_posterior("rgrgr_r94", s, mp, tw, tb, lg); }
extern "C" scrappie_matrix nanonet_rgrgr_r941_posterior(const raw_table s, float mp, float tw, float tb, bool lg) { return named_posterior("rgrgr_r941", s, mp, tw, tb, lg); }
extern "C" scrappie_matrix nanonet_rgrgr_r10_posterior(const raw_table s, float mp, float tw, float tb, bool lg) { return named_posterior("rgrgr_r10", s, mp, tw, tb, lg); }
extern "C" scrappie_matrix nanonet_rnnrf_r94_transitions(const raw_table s, float mp, float tw, float tb, bool lg) { return named_posterior("rnnrf_r94", s, mp, tw, tb, lg); }

extern "C" posterior_function_ptr get_posterior_function(const enum raw_model_type model) {
    switch (model) {
    case SCRAPPIE_MODEL_RAW: return nanonet_raw_posterior;
    case SCRAPPIE_MODEL_RGRGR_R9_4: return nanonet_rgrgr_r94_posterior;
    case SCRAPPIE_MODEL_RGRGR_R9_4_1: return nanonet_rgrgr_r941_posterior;
    case SCRAPPIE_MODEL_RGRGR_R10: return nanonet_rgrgr_r10_posterior;
    case SCRAPPIE_MODEL_RNNRF_R9_4: return nanonet_rnnrf_r94_transitions;
    default:
        /* the reference errx()'s on an invalid enum (networks.c:120-123) */
        fprintf(stderr, "scrappie_hip: model enum %d has no posterior function\n", (int)model);
        exit(EXIT_FAILURE);
    }
}

extern "C" int get_raw_model_stride(const enum raw_model_type model) {
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    const int h = default_model(e, raw_model_string(model));
    return h < 0 ? -1 : e->models[h]->stride;
}

extern "C" int get_raw_model_stride_from_string(const char *modelstr) {      /* python/build.py:34-44 */
    const enum raw_model_type t = get_raw_model(modelstr);
    if (t == SCRAPPIE_MODEL_INVALID) return -1;
    return get_raw_model_stride(t);
}

/* decode_transducer (decode.c:123 on host posteriors; the other half of the reference's per-read loop body, scrappie_raw.c:279-287), from many host threads
 * at once: the calls that are waiting run as one launch -- one workgroup per read, a tile whose 16 lanes all alias that read's columns (strideB = 0), so a
 * call's path and score do not depend on its company; a call with the queue off is the same launch with one read.  The posteriors are 3.3 MB per read of
 * 4000 samples: every caller of the queue copies its own into pinned memory (all at once), one transfer takes them to the device. */
struct DecReq {
    const_scrappie_matrix post = nullptr;
    float stay_pen = 0.f, skip_pen = 0.f, local_pen = 0.f;
    bool slip = false;
    int *seq = nullptr;
    float score = NAN;
    int phase = 0;                  /* 0 queued, 1 asked to copy its posterior to `dst`, 2 copied, 3 done */
    float *dst = nullptr;
};
/* the queue's pinned input buffer: sized by the leader, filled by the members of the launch in preparation (one leader at a time), read by that launch.
 * The queue has static storage and an HBuf frees its memory when it is destroyed, so the buffer lives behind a reference to an object that is never
 * deleted: no HIP call while the process exits (the process-default engine is never destroyed for the same reason).  g_co and g_cc hold no buffer. */
struct DecCoalescer : ShCoalescer<DecReq> { HBuf &stage = *new HBuf; };
static DecCoalescer g_dc;

/* The requests share shape and penalties.  `staged`: their posteriors concatenated in pinned memory, read k at the column offset the reads before it add up
 * to (the queue's members have put them there); nullptr: they are copied into the engine's own staging buffer here, under its lock.  Results into the requests. */
static void decode_batch(scrappie_hip_engine *e, std::vector<DecReq *> &reqs, const float *staged) {
    const size_t n = reqs.size();
    const DecReq *f = reqs[0];
    const int NH = (int)f->post->nr - 1, NQ = NH / 4;
    const size_t stride = f->post->stride;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    const size_t npad = 16 * n;
    long long ncb = 0;
    for (const DecReq *r : reqs) ncb += (long long)r->post->nc;
    /* metadata: sig_off[npad] | seq_off[npad] | (unused)[npad] | tile_boff[n] | rN[npad] | rT[npad] | tile_T[n] */
    std::vector<char> hm(npad * 24 + n * 8 + npad * 8 + n * 4, 0);
    long long *seq_off = (long long *)(hm.data() + npad * 8);
    long long *tboff = (long long *)(hm.data() + npad * 24);
    int *rN = (int *)(hm.data() + npad * 24 + n * 8), *rT = rN + npad, *tT = rT + npad;
    long long nseq = 0, boff = 0;
    for (size_t k = 0; k < n; k++) {
        const int T = (int)reqs[k]->post->nc;
        tboff[k] = boff; tT[k] = T;
        /* every lane of the tile reads the same columns (strideB = 0) and runs the read; lane 0's path is walked back */
        for (int b = 0; b < 16; b++) { rN[k * 16 + b] = 1; rT[k * 16 + b] = T; seq_off[k * 16 + b] = nseq; }
        nseq += T + 1; boff += T;
    }
    /* (grow-only, kept between launches: seven hipMalloc / hipFree pairs per launch cost more than the transfer) */
    DBuf &dmeta = e->d_dec[0], &dpost = e->d_dec[1], &dtb = e->d_dec[2], &dtbe = e->d_dec[3], &dfs = e->d_dec[4], &dfsc = e->d_dec[5], &dseq = e->d_dec[6];
    bool ok = false;
    do {
        const size_t pbytes = (size_t)ncb * stride * 4;
        if (dmeta.ensure(hm.size()) || dpost.ensure(pbytes) || dtb.ensure((size_t)ncb * NQ * 16 * 4) || dtbe.ensure((size_t)ncb * 16 * 4) ||
            dfs.ensure(npad * 4) || dfsc.ensure(npad * 4) || dseq.ensure((size_t)nseq * 4) || e->h_dec_out.ensure((size_t)nseq * 4 + npad * 4)) break;
        if (!staged) {
            if (e->h_dec_in.ensure(pbytes)) break;
            float *h = e->h_dec_in.as<float>();
            for (size_t k = 0; k < n; k++) memcpy(h + (size_t)tboff[k] * stride, reqs[k]->post->data.f, (size_t)reqs[k]->post->nc * stride * 4);
            staged = h;
        }
        if (hipMemcpyAsync(dmeta.p, hm.data(), hm.size(), hipMemcpyHostToDevice, s) != hipSuccess) break;
        if (hipMemcpyAsync(dpost.p, staged, pbytes, hipMemcpyHostToDevice, s) != hipSuccess) break;
        char *d = dmeta.as<char>();
        ShMeta md;
        md.sig_off = (const unsigned long long *)d;
        md.tile_boff = (const long long *)(d + npad * 24);
        md.rN = (const int *)(d + npad * 24 + n * 8);
        md.rT = md.rN + npad;
        md.tile_T = md.rT + npad;
        ShVitArgs va;
        va.E = dpost.as<float>(); va.sums = nullptr;
        va.strideT = (long long)stride; va.strideQ = 4; va.strideB = 0;
        va.want_log = 0; va.min_prob = 0.f;
        va.stay_pen = f->stay_pen; va.skip_pen = f->skip_pen; va.local_pen = f->local_pen; va.use_slip = f->slip ? 1 : 0;
        va.tb = dtb.as<unsigned>(); va.tb_end = dtbe.as<int>();
        va.final_state = dfs.as<int>(); va.final_score = dfsc.as<float>();
        va.hp_side = nullptr; va.hp_off = nullptr; va.dbg = nullptr; va.dump_final = 0;
        va.seg = nullptr; va.lane_off = nullptr; va.vstate = nullptr; va.flag = nullptr; va.err = nullptr;   /* one workgroup per read, the whole tile */
        if (launch_viterbi(s, NH, va, md, n)) break;
        /* lane 0 of every tile: the other lanes hold the same path */
        hipLaunchKernelGGL(k_backtrace_lane0, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, dtb.as<unsigned>(), dtbe.as<int>(), dfs.as<int>(), md,
                           (const long long *)(d + npad * 8), dseq.as<int>(), (int)n, NQ);
        int *hseq = e->h_dec_out.as<int>();
        if (hipMemcpyAsync(hseq, dseq.p, (size_t)nseq * 4, hipMemcpyDeviceToHost, s) != hipSuccess) break;
        if (hipMemcpyAsync(hseq + nseq, dfsc.p, npad * 4, hipMemcpyDeviceToHost, s) != hipSuccess) break;
        if (sh_stream_wait(s) != hipSuccess) break;
        const float *hsc = (const float *)(hseq + nseq);
        for (size_t k = 0; k < n; k++) {
            memcpy(reqs[k]->seq, hseq + seq_off[k * 16], ((size_t)reqs[k]->post->nc + 1) * 4);
            reqs[k]->score = hsc[k * 16];
        }
        ok = true;
    } while (0);
    if (!ok) { (void)hipGetLastError(); for (DecReq *r : reqs) r->score = NAN; }
}

static float coalesced_decode(scrappie_hip_engine *e, const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen, int *seq, bool allow_slip) {
    constexpr size_t MAX_READS = 1024;
    constexpr long long MAX_BLOCKS = 200000;                          /* 16 KB of traceback + 4 KB of posterior per block */
    ShInside inside(g_presence);
    DecReq r;
    r.post = logpost; r.stay_pen = stay_pen; r.skip_pen = skip_pen; r.local_pen = local_pen; r.slip = allow_slip; r.seq = seq;
    g_dc.run(r, g_presence, MAX_READS, true,
        [&](std::deque<DecReq *> &q, std::vector<DecReq *> &batch) {
            take_compatible(q, batch, MAX_READS, MAX_BLOCKS,
                            [](const DecReq *f, const DecReq *c) {
                                return c->post->nr == f->post->nr && c->post->stride == f->post->stride && c->stay_pen == f->stay_pen && c->skip_pen == f->skip_pen &&
                                       c->local_pen == f->local_pen && c->slip == f->slip;
                            },
                            [](const DecReq *c) { return (long long)c->post->nc; });
        },
        [&](std::vector<DecReq *> &batch) {      /* every member copies its own posterior into the launch's pinned buffer, all at once */
            const size_t stride = batch[0]->post->stride;
            size_t ncb = 0;
            for (const DecReq *c : batch) ncb += c->post->nc;
            if (g_dc.stage.ensure(ncb * stride * 4) != 0) return false;
            float *at = g_dc.stage.as<float>();
            for (DecReq *c : batch) { c->dst = at; at += c->post->nc * stride; }
            return true;
        },
        [](DecReq &c) { memcpy(c.dst, c.post->data.f, (size_t)c.post->nc * c.post->stride * 4); },
        [&](std::vector<DecReq *> &batch) { decode_batch(e, batch, g_dc.stage.as<float>()); });
    return r.score;
}
extern "C" void scrappie_hip_decode_coalescer_stats(unsigned long long out[3]) {
    std::lock_guard<std::mutex> lk(g_dc.mu);
    out[0] = g_dc.n_batches; out[1] = g_dc.n_reads; out[2] = g_dc.max_batch;
    if (getenv("SCRAPPIE_HIP_COALESCE_TIMES")) fprintf(stderr, "decode coalescer: %llu launches took %.1f ms in all\n", g_dc.n_batches, g_dc.service_us / 1e3);
}

extern "C" float decode_transducer(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen, int *seq, bool allow_slip) {
    if (!logpost || !seq) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    const int NH = (int)logpost->nr - 1, T = (int)logpost->nc;
    if (NH % 64 != 0 || (allow_slip && NH % 256 != 0) || T <= 0) return NAN;
    if (NH != 64 && NH != 256 && NH != 1024) return NAN;
    if (coalesce_on('d')) return coalesced_decode(e, logpost, stay_pen, skip_pen, local_pen, seq, allow_slip);
    DecReq r;
    r.post = logpost; r.stay_pen = stay_pen; r.skip_pen = skip_pen; r.local_pen = local_pen; r.slip = allow_slip; r.seq = seq;
    std::vector<DecReq *> one{&r};
    decode_batch(e, one, nullptr);
    return r.score;
}

/* decode_crf (decode.c:836 on host transition matrices): the serial recursion of a read on one thread, a thread per read -- the waiting calls of many host
 * threads in one launch (coalesced like decode_transducer), or one call with the queue off */
__global__ void k_crf_viterbi_batch(const float *__restrict__ trans, int stride, const long long *__restrict__ coff, const int *__restrict__ Ts, int n,
                                    unsigned *__restrict__ tbbuf, int *__restrict__ path, float *__restrict__ score) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int T = Ts[r];
    const float *tr0 = trans + coff[r] * stride;
    unsigned *tb = tbbuf + coff[r];
    int *pth = path + coff[r] + r;                     /* T + 1 entries per read */
    float prev[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, curr[5];
    for (int t = 0; t < T; t++) {
        const float *tr = tr0 + (long long)t * stride;
        unsigned pack = 0;
        for (int to = 0; to < 5; to++) {
            float best = tr[to * 5] + prev[0];
            unsigned from = 0;
            for (int fr = 1; fr < 5; fr++) {
                const float sc = tr[to * 5 + fr] + prev[fr];
                if (sc > best) { best = sc; from = fr; }
            }
            curr[to] = best;
            pack |= from << (3 * to);
        }
        tb[t] = pack;
        for (int i = 0; i < 5; i++) prev[i] = curr[i];
    }
    float best = prev[0];
    int arg = 0;
    for (int i = 1; i < 5; i++) if (prev[i] > best) { best = prev[i]; arg = i; }
    score[r] = best;
    pth[T] = arg;
    for (int blk = T; blk > 0; blk--) { arg = (tb[blk - 1] >> (3 * arg)) & 7u; pth[blk - 1] = arg; }
}

struct CrfReq { const_scrappie_matrix trans = nullptr; int *path = nullptr; float score = NAN; int phase = 0; };
static ShCoalescer<CrfReq> g_cc;

static void crf_batch(scrappie_hip_engine *e, std::vector<CrfReq *> &reqs) {
    const size_t n = reqs.size(), stride = reqs[0]->trans->stride;
    long long ncol = 0;
    for (CrfReq *r : reqs) ncol += (long long)r->trans->nc;
    /* pinned input: [transitions of all reads][column offset per read][T per read] */
    const size_t fbytes = (size_t)ncol * stride * 4, in_bytes = fbytes + n * 8 + n * 4;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    DBuf &din = e->d_crf[0], &dtb = e->d_crf[1], &dpath = e->d_crf[2], &dsc = e->d_crf[3];
    bool ok = false;
    do {
        if (e->h_crf_in.ensure(in_bytes) || e->h_crf_out.ensure(((size_t)ncol + n) * 4 + n * 4) || din.ensure(in_bytes) || dtb.ensure((size_t)ncol * 4) ||
            dpath.ensure(((size_t)ncol + n) * 4) || dsc.ensure(n * 4)) break;
        char *h = e->h_crf_in.as<char>();
        long long *coff = (long long *)(h + fbytes);
        int *Ts = (int *)(h + fbytes + n * 8);
        long long c = 0;
        for (size_t k = 0; k < n; k++) {
            const size_t T = reqs[k]->trans->nc;
            memcpy(h + (size_t)c * stride * 4, reqs[k]->trans->data.f, T * stride * 4);
            coff[k] = c; Ts[k] = (int)T; c += (long long)T;
        }
        hipStream_t s = e->stream;
        if (hipMemcpyAsync(din.p, h, in_bytes, hipMemcpyHostToDevice, s) != hipSuccess) break;
        const char *d = din.as<char>();
        hipLaunchKernelGGL(k_crf_viterbi_batch, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const float *)d, (int)stride, (const long long *)(d + fbytes),
                           (const int *)(d + fbytes + n * 8), (int)n, dtb.as<unsigned>(), dpath.as<int>(), dsc.as<float>());
        int *hp = e->h_crf_out.as<int>();
        if (hipMemcpyAsync(hp, dpath.p, ((size_t)ncol + n) * 4, hipMemcpyDeviceToHost, s) != hipSuccess) break;
        if (hipMemcpyAsync(hp + ncol + n, dsc.p, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess) break;
        if (sh_stream_wait(s) != hipSuccess) break;
        const float *hs = (const float *)(hp + ncol + n);
        for (size_t k = 0; k < n; k++) {
            memcpy(reqs[k]->path, hp + coff[k] + (long long)k, ((size_t)Ts[k] + 1) * 4);
            reqs[k]->score = hs[k];
        }
        ok = true;
    } while (0);
    if (!ok) { (void)hipGetLastError(); for (CrfReq *r : reqs) r->score = NAN; }
}

static float coalesced_decode_crf(scrappie_hip_engine *e, const_scrappie_matrix trans, int *path) {
    constexpr size_t MAX_READS = 4096;
    constexpr long long MAX_COLS = 4000000;
    ShInside inside(g_presence);
    CrfReq r;
    r.trans = trans; r.path = path;
    g_cc.run(r, g_presence, MAX_READS, false,
        [&](std::deque<CrfReq *> &q, std::vector<CrfReq *> &batch) {
            take_compatible(q, batch, MAX_READS, MAX_COLS, [](const CrfReq *f, const CrfReq *c) { return c->trans->stride == f->trans->stride; },
                            [](const CrfReq *c) { return (long long)c->trans->nc; });
        },
        [](std::vector<CrfReq *> &) { return true; }, [](CrfReq &) {},
        [&](std::vector<CrfReq *> &batch) { crf_batch(e, batch); });
    return r.score;
}
extern "C" void scrappie_hip_crf_coalescer_stats(unsigned long long out[3]) {
    std::lock_guard<std::mutex> lk(g_cc.mu);
    out[0] = g_cc.n_batches; out[1] = g_cc.n_reads; out[2] = g_cc.max_batch;
}

extern "C" float decode_crf(const_scrappie_matrix trans, int *path) {
    if (!trans || !path) return NAN;
    if (trans->nr != 25 || trans->nc == 0) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    if (coalesce_on('d')) return coalesced_decode_crf(e, trans, path);
    CrfReq r;
    r.trans = trans; r.path = path;
    std::vector<CrfReq *> one{&r};
    crf_batch(e, one);
    return r.score;
}
