/* sh_eng_crfpost.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * base probabilities of the flip-flop models (k_crf_post, sh_crf_post.h).  Two ways in.  Inside a launch group of scrappie_hip_basecall_batch_probs
 * (crf_post_enqueue / crf_post_download / crf_post_deliver, called by the stages of run_pipeline and by stitch_group): the kernel's tiled form on the
 * transitions k_crf<true> has left in d_E, into the slot's own buffer, home on the copy stream.  And scrappie_hip_posterior_crf_batch on host
 * matrices: upload, the reference-layout form, download, cut into launches by a column budget.  The host's share -- the plan, the staging, a result
 * matrix -- is C (sh_host.c). */

static std::atomic<uint64_t> g_crf_post_launches;
extern "C" uint64_t scrappie_hip_crf_post_launch_count(void) { return g_crf_post_launches.load(std::memory_order_relaxed); }
extern "C" void scrappie_hip_crf_post_timing(scrappie_hip_engine *e, double out[3]) { timing3(e ? e->crf_post_ms : nullptr, out); }

/* ------------------------------------------------------------------ */
/* inside a launch group                                                */
/* ------------------------------------------------------------------ */
/* the timing marks of a group that returns probabilities: events of the slot's own, made on first use */
enum { PEV_MAIN = 0, PEV_POST, PEV_POST_END, PEV_COPY, PEV_COPY_END, PEV_COUNT };
static int crf_post_mark(Slot &sl, int k, hipStream_t st) {
    if (!sl.pev[k]) HIPCHK(hipEventCreate(&sl.pev[k]));
    HIPCHK(hipEventRecord(sl.pev[k], st));
    return 0;
}

/* behind k_crf<true> on the main stream (d_E belongs to the engine: the next group's output layer overwrites it) */
static int crf_post_enqueue(Slot &sl, GroupRun &c) {
    scrappie_hip_engine *e = c.e;
    LaunchGroup &lg = sl.lg;
    const hipStream_t s = c.s;
    std::vector<size_t> nb(lg.npad);
    for (size_t i = 0; i < lg.npad; i++) nb[i] = (size_t)std::max(lg.rT[i], 0);
    lg.post_off.resize(lg.npad);
    lg.npost = scrappie_hip_crf_post_plan(nb.data(), lg.npad, lg.post_off.data());
    const size_t tot = (size_t)lg.npost;
    if (sl.h_postoff.ensure(lg.npad * 8) || sl.d_postoff.ensure(lg.npad * 8) || sl.d_post.ensure((tot + 128) * 4) || sl.h_post.ensure(std::max<size_t>(tot, 1) * 4)) return -1;
    memcpy(sl.h_postoff.p, lg.post_off.data(), lg.npad * 8);        /* (pinned, the slot's: not written again before the group is collected) */
    hipLaunchKernelGGL(k_upload_words, dim3((unsigned)((lg.npad / 2 + 255) / 256)), dim3(256), 0, s, (const u32x4 *)sl.h_postoff.p, sl.d_postoff.as<u32x4>(), (long long)(lg.npad / 2));
    if (e->ev_ok && crf_post_mark(sl, PEV_POST, s)) return -1;
    g_crf_post_launches.fetch_add(1, std::memory_order_relaxed);
    if (launch_k<k_crf_post<ShCrfTiled>>(dim3((unsigned)(lg.npad / 16)), dim3(128), 0, s, ShCrfTiled{e->d_E.as<float>(), c.mp.md.tile_boff}, c.mp.md.rT, c.mp.md.tile_T,
                                         (const long long *)sl.d_postoff.p, sl.d_post.as<float>(), sl.d_post.as<float>() + tot)) return -1;
    if (e->ev_ok && crf_post_mark(sl, PEV_POST_END, s)) return -1;
    return 0;
}

/* on the copy stream, behind the slot's result transfer and in front of its done event */
static int crf_post_download(Slot &sl, GroupRun &c) {
    const LaunchGroup &lg = sl.lg;
    if (c.e->ev_ok && crf_post_mark(sl, PEV_COPY, c.cs)) return -1;
    if (lg.npost > 0) HIPCHK(hipMemcpyAsync(sl.h_post.p, sl.d_post.p, (size_t)lg.npost * 4, hipMemcpyDeviceToHost, c.cs));
    if (c.e->ev_ok && crf_post_mark(sl, PEV_COPY_END, c.cs)) return -1;
    return 0;
}

/* the group is done and stitched: a matrix for every read that has a call (out[] in the group's own order), the group's times onto the call's */
static void crf_post_deliver(scrappie_hip_engine *e, Slot &sl, const scrappie_hip_call *out) {
    const LaunchGroup &lg = sl.lg;
    auto part = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            const int o = lg.order[i];
            if (o < 0 || lg.rT[i] <= 0 || !out[o].basecall || !lg.post.dst[(size_t)o]) continue;
            *lg.post.dst[(size_t)o] = sh_crf_post_take(sl.h_post.as<float>() + lg.post_off[i], (size_t)lg.rT[i]);
        }
    };
    /* 10 000 matrices of 800 blocks are 160 MB out of pinned memory into containers of their own: tens of ms on one thread, so on a few, as the stitching */
    unsigned nthr = std::min(host_threads(), 8u);
    if (e->host_thread_budget) nthr = std::min(nthr, e->host_thread_budget);
    if (lg.npad < 256 || nthr < 2) part(0, lg.npad);
    else {
        std::vector<std::thread> th;
        const size_t per = (lg.npad + nthr - 1) / nthr;
        for (size_t lo = 0; lo < lg.npad; lo += per) th.emplace_back(part, lo, std::min(lg.npad, lo + per));
        for (auto &x : th) x.join();
    }
    if (!e->ev_ok) return;
    const int span[3][2] = {{PEV_MAIN, PEV_POST}, {PEV_POST, PEV_POST_END}, {PEV_COPY, PEV_COPY_END}};
    for (int k = 0; k < 3; k++) {
        float ms = 0.0f;
        if (sl.pev[span[k][0]] && sl.pev[span[k][1]] && hipEventElapsedTime(&ms, sl.pev[span[k][0]], sl.pev[span[k][1]]) == hipSuccess) e->crf_post_ms[k] += ms;
        else (void)hipGetLastError();
    }
}

extern "C" int scrappie_hip_basecall_batch_probs(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n, const scrappie_hip_params *p,
                                                 scrappie_hip_call *out, scrappie_matrix *probs) {
    if (!e || (n && (!reads || !out || !probs))) return set_err("basecall_batch_probs: null argument");
    Model *m = get_model(e, model);
    if (!m) return -1;
    if (m->arch != 1) return set_err("basecall_batch_probs: model '%s' is not a CRF (flip-flop) model: base probabilities are the posterior over its five states", m->name.c_str());
    for (size_t i = 0; i < n; i++) probs[i] = nullptr;
    std::lock_guard<std::mutex> lk(e->call_mu);
    for (double &x : e->crf_post_ms) x = 0.0;
    const int rc = basecall_batch_one(e, model, reads, n, p, out, probs);
    if (rc) for (size_t i = 0; i < n; i++) probs[i] = free_scrappie_matrix(probs[i]);      /* a failed call returns nothing */
    return rc;
}

/* ------------------------------------------------------------------ */
/* on host matrices                                                     */
/* ------------------------------------------------------------------ */
/* one launch over the matrices who[] of the call */
static int crf_post_run(scrappie_hip_engine *e, const std::vector<size_t> &who, const const_scrappie_matrix *trans, scrappie_matrix *out) {
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = who.size(), ntile = (n + 15) / 16, npad = ntile * 16;
    /* longest first, so that the 16 reads of a workgroup are of a length; the output keeps the call's order (the plan's) */
    std::vector<size_t> order(who);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return trans[a]->nc > trans[b]->nc; });
    std::vector<size_t> nb(npad, 0);
    for (size_t k = 0; k < n; k++) nb[k] = trans[order[k]]->nc;
    std::vector<long long> ooff(npad);
    const size_t tot = (size_t)scrappie_hip_crf_post_plan(nb.data(), npad, ooff.data());
    size_t nfl = 0;
    for (size_t k = 0; k < n; k++) nfl += trans[order[k]]->nc * trans[order[k]]->stride;
    nfl = (nfl + 1) & ~(size_t)1;
    /* pinned input: [transitions][first float i64 npad][output offset i64 npad][stride i32 npad][blocks i32 npad][tile blocks i32 ntile], one upload */
    const size_t in_bytes = nfl * 4 + npad * 24 + ntile * 4;
    if (e->h_cp_in.ensure(in_bytes) || e->d_cp_in.ensure(in_bytes) || e->d_cp_out.ensure((tot + 128) * 4) || e->h_cp_out.ensure(tot * 4)) return -1;
    char *h = e->h_cp_in.as<char>();
    long long *foff = (long long *)(h + nfl * 4), *hoff = foff + npad;
    int *stride = (int *)(hoff + npad), *T = stride + npad, *tile_T = T + npad;
    (void)sh_crf_post_stage(trans, order.data(), n, npad, (float *)h, foff, stride, T, tile_T);
    memcpy(hoff, ooff.data(), npad * 8);
    HIPCHK(hipMemcpyAsync(e->d_cp_in.p, h, in_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(sh_stream_wait(s));
    const auto t1 = std::chrono::steady_clock::now();
    const char *d = e->d_cp_in.as<char>();
    const size_t o_w = nfl * 4;
    g_crf_post_launches.fetch_add(1, std::memory_order_relaxed);
    if (launch_k<k_crf_post<ShCrfRef>>(dim3((unsigned)ntile), dim3(128), 0, s, ShCrfRef{(const float *)d, (const long long *)(d + o_w), (const int *)(d + o_w + npad * 16)},
                                       (const int *)(d + o_w + npad * 20), (const int *)(d + o_w + npad * 24), (const long long *)(d + o_w + npad * 8),
                                       e->d_cp_out.as<float>(), e->d_cp_out.as<float>() + tot)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    const auto t2 = std::chrono::steady_clock::now();
    const float *ho = e->h_cp_out.as<float>();
    HIPCHK(hipMemcpyAsync(e->h_cp_out.p, e->d_cp_out.p, tot * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    for (size_t k = 0; k < n; k++) {
        out[order[k]] = sh_crf_post_take(ho + ooff[k], nb[k]);
        if (!out[order[k]]) return set_err("out of host memory");
    }
    const auto t3 = std::chrono::steady_clock::now();
    e->crf_post_ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    e->crf_post_ms[1] += std::chrono::duration<double, std::milli>(t2 - t1).count();
    e->crf_post_ms[2] += std::chrono::duration<double, std::milli>(t3 - t2).count();
    return 0;
}

extern "C" int scrappie_hip_posterior_crf_batch(scrappie_hip_engine *e, const const_scrappie_matrix *trans, size_t n, scrappie_matrix *out) {
    if (!e || (n && (!trans || !out))) return set_err("posterior_crf_batch: null argument");
    for (size_t i = 0; i < n; i++) out[i] = nullptr;
    (void)hipSetDevice(e->device);
    { std::lock_guard<std::mutex> lk(e->mu); for (double &x : e->crf_post_ms) x = 0.0; }
    constexpr size_t MAX_COLS = 4000000, MAX_READS = 1u << 20;      /* as decode_crf's batch: what one launch stages in pinned memory */
    struct Load { size_t cols = 0, reads = 0; };
    LaunchCut<Load> cut{e, "posterior_crf_batch"};
    cut.run = [&](const std::vector<size_t> &who, Load &) { return crf_post_run(e, who, trans, out); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (!sh_crf_post_ok(trans[i]) || trans[i]->nc > (size_t)INT32_MAX / 64) {
            cut.refuse(i, "posterior_crf_batch: not a transition matrix of 25 rows and at least one block");
            continue;
        }
        cut.add(i, cut.load.cols + trans[i]->nc <= MAX_COLS && cut.load.reads < MAX_READS);
        cut.load.cols += trans[i]->nc; cut.load.reads++;
    }
    return cut.finish([&] { for (size_t i = 0; i < n; i++) out[i] = free_scrappie_matrix(out[i]); },
                      [](size_t i, const char *why) { set_err("%s (matrix %zu of the call)", why, i); });
}
