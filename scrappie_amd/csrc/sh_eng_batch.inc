/* sh_eng_batch.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * chain-bound reads on a helper engine, host-signal entry points, several GPUs. */

/* Chain-bound reads.  A read is a serial chain -- five recurrent layers of alternating direction, then the decoder, the traceback
 * walk and the stitching: SH_CHAIN_NS per block, whatever else the device does -- so a launch group lasts at least as long as its
 * longest read, and a call whose length distribution has a long tail spends most of its time with a few workgroups stepping and the
 * rest of the device idle (profiles/r3_long_tail.txt: 24 000 reads of lognormal(20 000, 0.8) samples, one of 400 000: 912 ms of
 * chain for 470 ms of work).  The reads whose own chain is longer than what the whole call would take at the device's full
 * rate are "long": scrappie_hip_basecall_batch runs them on a helper engine of the same device (its own streams and arenas), beside
 * the launch groups of all the others, so that the call lasts max(longest chain, work) instead of their sum.  Host only:
 * is_long[n] gets 0 / 1; returns the number of long reads (0: do not split).  The reference's schedule(dynamic) loop over whole
 * reads (scrappie_raw.c:355-400) has the same effect on a CPU: a long read occupies one thread while the others go on. */
#ifndef SH_CHAIN_NS
#define SH_CHAIN_NS 11400.0     /* per block of one read: 5 x 1.29 us of recurrent layer + 5.3 decoder + 0.92 traceback walk + 0.34 stitching (lone tiles) */
#endif
#ifndef SH_WORK_NS
#define SH_WORK_NS 3.5          /* per block and read with the device full: 27.9 ms per 10 000 x 800 */
#endif
extern "C" long scrappie_hip_plan_tail(const uint32_t *lengths, size_t n, int stride, size_t max_long_blocks, unsigned char *is_long) {
    if ((!lengths && n) || stride < 1 || !is_long) return -1;
    memset(is_long, 0, n);
    if (n < 2) return 0;
    double W = 0;
    std::vector<uint32_t> T(n);
    for (size_t i = 0; i < n; i++) { T[i] = (uint32_t)(((unsigned long long)lengths[i] + stride - 1) / stride); W += T[i]; }
    const double thr = std::max(4096.0, W * SH_WORK_NS / SH_CHAIN_NS);             /* blocks; never below ~20 000 samples */
    std::vector<uint32_t> cand;
    for (size_t i = 0; i < n; i++) if ((double)T[i] > thr) cand.push_back((uint32_t)i);
    if (cand.empty() || cand.size() == n) return 0;
    std::stable_sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) { return T[a] > T[b]; });
    /* the longest first, as long as they fit the helper's arena in ONE launch group (tiles of 16: blocks of a tile = its longest read's)
     * and stay a small part of the call: a second group would add its own chain, and a call of mostly long reads has no tail to hide */
    double blocks = 0, work = 0;
    long cnt = 0;
    for (size_t k = 0; k < cand.size(); k++) {
        if (k % 16 == 0) { if (max_long_blocks && blocks + T[cand[k]] > (double)max_long_blocks) break; blocks += T[cand[k]]; }
        if (work + T[cand[k]] > 0.15 * W) break;
        work += T[cand[k]];
        is_long[cand[k]] = 1; cnt++;
    }
    return cnt;
}

/* (probs: scrappie_hip_basecall_batch_probs -- every launch group returns its reads' base probabilities as well, sh_eng_crfpost.inc) */
static int basecall_batch_one(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out,
                              scrappie_matrix *probs = nullptr);

/* The helper's share of the device's memory: its launch groups last as long as their longest read whatever they hold, so its rate is
 * its arena per chain.  0.3 against 0.15: a stream of 24 calls of 12 000 lognormal reads 1.19e9 against 1.10e9 samples/s
 * (profiles/r5_long_tail.txt).  SCRAPPIE_HIP_TAIL_MEM overrides (0 .. 0.4]; two helpers (SCRAPPIE_HIP_TAIL=2) get 0.15 each. */
static bool tail_two_helpers();
static double tail_mem_frac() {
    static const double f = [] { const char *v = getenv("SCRAPPIE_HIP_TAIL_MEM"); const double x = v ? atof(v) : 0; return x > 0 && x <= 0.4 ? x : (tail_two_helpers() ? 0.15 : 0.3); }();
    return f;
}
static bool tail_two_helpers() {
    /* SCRAPPIE_HIP_TAIL=2: a second helper when the first is busy.  Measured SLOWER on a stream of long-tailed calls (24 x 12 000 lognormal reads:
     * 7.3e8 against 8.7e8 samples/s, profiles/r4_long_tail.txt): two chain-bound groups hold twice the CUs and each serves fewer tickets */
    static const bool on = [] { const char *v = getenv("SCRAPPIE_HIP_TAIL"); return v && atoi(v) == 2; }();
    return on;
}
static bool tail_enabled(const scrappie_hip_engine *e) {
    if (e->is_tail) return false;
    if (e->tail_mode >= 0) return e->tail_mode != 0;
    static const bool env_on = [] { const char *v = getenv("SCRAPPIE_HIP_TAIL"); return !(v && atoi(v) == 0); }();
    return env_on;
}

/* a helper engine: same device, same models at the same indices, same settings */
static scrappie_hip_engine *make_helper(scrappie_hip_engine *e) {
    scrappie_hip_engine *t = scrappie_hip_engine_create(e->device);
    if (!t) return nullptr;
    t->is_tail = true;
    for (const auto &b : e->blobs) {
        t->dbg_force_f32 = b.force_f32;
        const int want = scrappie_hip_find_model(e, b.name.c_str());
        if (load_model_mem_one(t, b.name.c_str(), b.bytes.data(), b.bytes.size()) != want) { scrappie_hip_engine_destroy(t); set_err("helper engine: model '%s' did not load at index %d", b.name.c_str(), want); return nullptr; }
    }
    return t;
}
static void sync_helper(scrappie_hip_engine *e, scrappie_hip_engine *t) {
    t->handover = e->handover; t->max_launch_reads = e->max_launch_reads; t->max_launch_blocks = e->max_launch_blocks;
    t->dbg_ff_separate = e->dbg_ff_separate; t->dbg_fv_single = e->dbg_fv_single; t->dbg_gru32 = e->dbg_gru32; t->dbg_gru_tiles = e->dbg_gru_tiles; t->dbg_decoder_cus = e->dbg_decoder_cus; t->dbg_decoder_lanes = e->dbg_decoder_lanes; t->dbg_redo_all = e->dbg_redo_all;
    t->profiling = false;
}
static scrappie_hip_engine *tail_engine(scrappie_hip_engine *e) {
    if (!e->tail) {
        /* several arenas on one device: a helper's launch groups are a few long tiles.  The main engine's arenas only grow and may hold up to 0.70 of the
         * device from earlier calls that had no chain-bound reads, so the helper's share is what is actually FREE now (less a margin for its weights and the
         * preparers' slots), at most tail_mem_frac(); with no room to speak of calls are simply not split any more (ADVICE r5: 0.70 + 0.30 did not fit) */
        (void)hipSetDevice(e->device);
        double frac = tail_mem_frac();
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && e->total_mem) frac = std::min(frac, 0.85 * (double)fr / (double)e->total_mem);
        if (e->dbg_tail_free_frac > 0) frac = std::min(frac, e->dbg_tail_free_frac);      /* (test hook: pretend this much is free) */
        if (frac < 0.03) { e->tail_mode = 0; return nullptr; }
        e->tail = make_helper(e);
        if (!e->tail) return nullptr;
        e->mem_frac = 0.45; e->tail->mem_frac = frac; e->tail_frac = frac;
    }
    std::lock_guard<std::mutex> lk(e->tail_mu);           /* (a helper's settings change only while it is idle) */
    if (e->tail_busy == 0) {
        sync_helper(e, e->tail);
        if (e->tail2) sync_helper(e, e->tail2);
        if (e->dbg_fail_tail) { e->tail->dbg_fail_run = e->dbg_fail_tail; e->dbg_fail_tail = 0; }
    }
    return e->tail;
}

typedef std::shared_ptr<scrappie_hip_engine::TailTicket> TicketPtr;
static void tail_worker(scrappie_hip_engine *e, scrappie_hip_engine *helper) {
    for (;;) {
        std::unique_lock<std::mutex> lk(e->tail_mu);
        e->tail_cv.wait(lk, [&] { return e->tail_stop || !e->tail_q.empty(); });
        if (e->tail_q.empty()) break;                 /* (stop: what is queued is still served) */
        std::vector<TicketPtr> batch;
        const TicketPtr f = e->tail_q.front();
        while (!e->tail_q.empty() && e->tail_q.front()->model == f->model && memcmp(&e->tail_q.front()->p, &f->p, sizeof f->p) == 0) {
            batch.push_back(e->tail_q.front());
            e->tail_q.pop_front();
        }
        e->tail_busy++;
        lk.unlock();
        std::vector<raw_table> all;
        for (const TicketPtr &t : batch) all.insert(all.end(), t->reads.begin(), t->reads.end());
        std::vector<scrappie_hip_call> calls(all.size());
        const int rc = basecall_batch_one(helper, f->model, all.data(), all.size(), &f->p, calls.data());
        const std::string err = rc ? std::string(g_err) : std::string();
        lk.lock();
        size_t at = 0;
        for (const TicketPtr &t : batch) {
            t->rc = rc; t->err = err;
            if (!rc) t->calls.assign(calls.begin() + (long)at, calls.begin() + (long)(at + t->reads.size()));
            at += t->reads.size();
            t->done = true;
        }
        e->n_tail_groups++;
        e->n_redo_tail += helper->n_redo; helper->n_redo = 0;
        e->tail_busy--;
        lk.unlock();
        e->tail_cv.notify_all();
    }
}
static TicketPtr tail_submit(scrappie_hip_engine *e, int model, const scrappie_hip_params &p, std::vector<raw_table> &&reads, std::vector<float> &&own = std::vector<float>()) {
    if (!e->tail2 && tail_two_helpers()) {
        bool busy;
        { std::lock_guard<std::mutex> lk(e->tail_mu); busy = e->tail_busy > 0 || !e->tail_q.empty(); }
        if (busy) {                                    /* the first helper has a group in hand: a second one for what comes now */
            scrappie_hip_engine *t2 = make_helper(e);
            if (t2) { t2->mem_frac = 0.15; sync_helper(e, t2); std::lock_guard<std::mutex> lk(e->tail_mu); e->tail2 = t2; }
            (void)hipSetDevice(e->device);
        }
    }
    TicketPtr t = std::make_shared<scrappie_hip_engine::TailTicket>();
    t->model = model; t->p = p; t->reads = std::move(reads);
    t->own = std::move(own);          /* (a vector's buffer moves with it: tables that point into it stay good) */
    {
        std::lock_guard<std::mutex> lk(e->tail_mu);
        t->id = e->tail_next++;
        e->tail_open[t->id] = t;
        e->tail_q.push_back(t);
        if (!e->tail_th_live) { e->tail_th = std::thread(tail_worker, e, e->tail); e->tail_th_live = true; }
        else if (e->tail2 && !e->tail_th2_live) { e->tail_th2 = std::thread(tail_worker, e, e->tail2); e->tail_th2_live = true; }
    }
    e->tail_cv.notify_all();
    return t;
}
static void tail_wait(scrappie_hip_engine *e, const TicketPtr &t) {
    std::unique_lock<std::mutex> lk(e->tail_mu);
    e->tail_cv.wait(lk, [&] { return t->done; });
}

/* what scrappie_hip_basecall_batch and _deferred share: lengths, the plan, the helper engine.  Returns the number of long reads (0: no
 * split), -1 on error */
static long tail_plan_len(scrappie_hip_engine *e, Model *m, const uint32_t *len, size_t n, std::vector<unsigned char> &is_long) {
    is_long.assign(n, 0);
    if (!tail_enabled(e) || n < 2 || e->alt_prob || e->alt_trunk || e->blobs.size() != e->models.size() || e->dbg_fail_run) return 0;
    const int unit = m->arch == 3 ? 1 : std::max(m->stride, 1);
    const size_t tail_cap = (size_t)((e->tail ? e->tail_frac : tail_mem_frac()) * (double)e->total_mem) / bytes_per_block(m, !decoder_fused(e, m));
    long nl = scrappie_hip_plan_tail(len, n, unit, e->max_launch_blocks ? e->max_launch_blocks : tail_cap, is_long.data());
    if (nl > 0 && !e->tail) {
        if (!tail_engine(e)) {
            if (tail_enabled(e)) return -1;
            is_long.assign(n, 0);                       /* no memory for a helper: the call runs whole on this engine */
            return 0;
        }
        if (e->tail_frac < tail_mem_frac() && !e->max_launch_blocks) {      /* a smaller helper than planned for: plan again */
            const size_t cap2 = (size_t)(e->tail_frac * (double)e->total_mem) / bytes_per_block(m, !decoder_fused(e, m));
            nl = scrappie_hip_plan_tail(len, n, unit, cap2, is_long.data());
        }
    }
    if (nl > 0 && !tail_engine(e)) return -1;
    return nl;
}
static long tail_plan(scrappie_hip_engine *e, Model *m, const raw_table *reads, size_t n, std::vector<unsigned char> &is_long) {
    const size_t per = m->arch == 3 ? (size_t)m->nfeat : 1;
    std::vector<uint32_t> len(n);
    for (size_t i = 0; i < n; i++) {
        const raw_table &rt = reads[i];
        len[i] = (uint32_t)(((rt.raw && rt.end > rt.start) ? rt.end - rt.start : 0) / per);
    }
    return tail_plan_len(e, m, len.data(), n, is_long);
}

/* scrappie_hip_basecall_batch that does not wait for the chain-bound reads: their calls are collected later (scrappie_hip_deferred_collect),
 * so that the NEXT call's launch groups run beside them too -- a stream of calls with long-tailed read lengths then runs at the
 * device's rate instead of one longest-read chain per call.  deferred[n] gets 1 for the reads whose out[] entry is still blank.
 * Returns a ticket (> 0) if any read was deferred, 0 if none, -1 on error.  The deferred reads' signals must stay valid until
 * their ticket has been collected. */
extern "C" long scrappie_hip_basecall_batch_deferred(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n,
                                                     const scrappie_hip_params *p, scrappie_hip_call *out, unsigned char *deferred) {
    if (!e || !reads || !out || !deferred) return set_err("basecall_batch_deferred: null argument");
    Model *m = get_model(e, model);
    if (!m) return -1;
    std::vector<unsigned char> is_long;
    const long nl = tail_plan(e, m, reads, n, is_long);
    if (nl < 0) return -1;
    memset(deferred, 0, n);
    if (nl == 0) return basecall_batch_one(e, model, reads, n, p, out) ? -1 : 0;
    std::vector<raw_table> rl, rr;
    std::vector<size_t> ir;
    for (size_t i = 0; i < n; i++) { if (is_long[i]) rl.push_back(reads[i]); else { rr.push_back(reads[i]); ir.push_back(i); } }
    scrappie_hip_params dp = scrappie_hip_default_params();
    const size_t nlong = rl.size();
    auto tk = tail_submit(e, model, p ? *p : dp, std::move(rl));
    std::vector<scrappie_hip_call> orr(rr.size());
    const int rc_main = basecall_batch_one(e, model, rr.data(), rr.size(), p, orr.data());
    for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].basecall = nullptr; out[i].basecall_length = 0; out[i].pos = nullptr; }
    if (rc_main) {                                    /* nothing is returned: the ticket is withdrawn */
        const std::string keep = g_err;
        tail_wait(e, tk);
        if (!tk->rc) scrappie_hip_free_calls(tk->calls.data(), tk->calls.size());
        { std::lock_guard<std::mutex> lk(e->tail_mu); e->tail_open.erase(tk->id); }
        return set_err("%s", keep.c_str());
    }
    for (size_t k = 0; k < ir.size(); k++) out[ir[k]] = orr[k];
    for (size_t i = 0; i < n; i++) deferred[i] = is_long[i];
    e->n_tail_calls++; e->n_tail_reads += nlong;
    return tk->id;
}
/* The same for signals that are already on the device (prepared there: scrappie_hip_prep_run): the few chain-bound reads are copied
 * back to host memory the ticket owns -- the helper engine stages from there, and the caller may reuse its device buffer as soon as
 * this call returns -- the others run from d_signal as scrappie_hip_basecall_device runs them. */
static long device_deferred(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets, const uint32_t *lengths, size_t n,
                            const scrappie_hip_params *p, scrappie_hip_call *out, unsigned char *deferred, bool stream);
extern "C" long scrappie_hip_basecall_device_deferred(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets,
                                                      const uint32_t *lengths, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out,
                                                      unsigned char *deferred) {
    return device_deferred(e, model, d_signal, offsets, lengths, n, p, out, deferred, false);
}
/* ... and streaming (scrappie_hip_basecall_device_stream): the call leaves its last launch group running; scrappie_hip_stream_pending
 * tells whether one is (0 / 1) */
extern "C" long scrappie_hip_basecall_device_deferred_stream(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets,
                                                             const uint32_t *lengths, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out,
                                                             unsigned char *deferred) {
    return device_deferred(e, model, d_signal, offsets, lengths, n, p, out, deferred, true);
}
extern "C" int scrappie_hip_stream_pending(scrappie_hip_engine *e) { return e && e->carry.live ? 1 : 0; }
static long device_deferred(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets, const uint32_t *lengths, size_t n,
                            const scrappie_hip_params *p, scrappie_hip_call *out, unsigned char *deferred, bool stream) {
    if (!e || !out || !deferred || (n && (!offsets || !lengths))) return set_err("basecall_device_deferred: null argument");
    Model *m = get_model(e, model);
    if (!m) return -1;
    std::vector<unsigned char> is_long;
    const long nl = m->arch == 3 ? 0 : tail_plan_len(e, m, lengths, n, is_long);
    if (nl < 0) return -1;
    memset(deferred, 0, n);
    if (nl == 0) return (stream ? scrappie_hip_basecall_device_stream(e, model, d_signal, offsets, lengths, n, p, out)
                                : scrappie_hip_basecall_device(e, model, d_signal, offsets, lengths, n, p, out)) ? -1 : 0;
    (void)hipSetDevice(e->device);
    TicketPtr tk;
    std::vector<uint64_t> off2; std::vector<uint32_t> len2; std::vector<size_t> ir;
    {
        size_t total = 0;
        for (size_t i = 0; i < n; i++) if (is_long[i]) total += lengths[i];
        std::vector<float> own(total);
        std::vector<raw_table> rl;
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            if (!is_long[i]) { off2.push_back(offsets[i]); len2.push_back(lengths[i]); ir.push_back(i); continue; }
            if (hipMemcpyAsync(own.data() + at, d_signal + offsets[i], (size_t)lengths[i] * 4, hipMemcpyDeviceToHost, e->ustream) != hipSuccess)      /* (the engine's own stream: the null stream would wait for the helper's group in flight) */
                return set_err("basecall_device_deferred: copying a chain-bound read back failed");
            rl.push_back(raw_table{nullptr, lengths[i], 0, lengths[i], own.data() + at});
            at += lengths[i];
        }
        HIPCHK(sh_stream_wait(e->ustream));
        scrappie_hip_params dp = scrappie_hip_default_params();
        tk = tail_submit(e, model, p ? *p : dp, std::move(rl), std::move(own));
    }
    /* the others as scrappie_hip_basecall_device(_stream) runs them, their calls straight into their places in out[] */
    for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].basecall = nullptr; out[i].basecall_length = 0; out[i].pos = nullptr; }
    int rc_main;
    {
        std::vector<uint64_t> goff[2];
        std::vector<uint32_t> glen[2];
        rc_main = run_groups(e, model, m, len2.data(), ir.size(), p, out, [&](int k, const uint32_t *idx, size_t cnt, GroupArgs &a) {
            goff[k].resize(cnt); glen[k].resize(cnt);
            for (size_t i = 0; i < cnt; i++) { goff[k][i] = off2[idx[i]]; glen[k][i] = len2[idx[i]]; }
            a.d = d_signal; a.off = goff[k].data(); a.len = glen[k].data();
            return 0;
        }, stream, ir.data());
    }
    if (rc_main) {                                    /* nothing is returned: the ticket is withdrawn */
        const std::string keep = g_err;
        tail_wait(e, tk);
        if (!tk->rc) scrappie_hip_free_calls(tk->calls.data(), tk->calls.size());
        { std::lock_guard<std::mutex> lk(e->tail_mu); e->tail_open.erase(tk->id); }
        return set_err("%s", keep.c_str());
    }
    for (size_t i = 0; i < n; i++) deferred[i] = is_long[i];
    e->n_tail_calls++; e->n_tail_reads += (unsigned long long)nl;
    return tk->id;
}
/* The calls of a ticket's deferred reads, in the order those reads had in their call.  wait = 0: returns -2 if they are not ready.
 * Returns their number, -1 on error (unknown ticket, out[] too small, or the helper's launch group failed: the ticket is gone). */
extern "C" long scrappie_hip_deferred_collect(scrappie_hip_engine *e, long ticket, scrappie_hip_call *out, size_t cap, int wait) {
    if (!e || !out) return set_err("deferred_collect: null argument");
    TicketPtr t;
    {
        std::lock_guard<std::mutex> lk(e->tail_mu);
        auto it = e->tail_open.find(ticket);
        if (it == e->tail_open.end()) return set_err("deferred_collect: no such ticket");
        t = it->second;
        if (!t->done && !wait) return -2;
    }
    tail_wait(e, t);
    (void)hipSetDevice(e->device);
    if (!t->rc && t->calls.size() > cap) return set_err("deferred_collect: %zu calls, room for %zu", t->calls.size(), cap);
    { std::lock_guard<std::mutex> lk(e->tail_mu); e->tail_open.erase(ticket); }
    if (t->rc) return set_err("%s", t->err.c_str());
    for (size_t k = 0; k < t->calls.size(); k++) out[k] = t->calls[k];
    return (long)t->calls.size();
}

/* Several host threads calling scrappie_hip_basecall_batch on ONE engine at once -- the reference's loop, `#pragma omp parallel for
 * schedule(dynamic)` over files (scrappie_raw.c:355,387), with a body that hands over 64 reads at a time (BASELINE config 2's "batch=64") --
 * share launch groups: a small call joins the queue of sh_coalesce.h, the calls that are waiting for the same engine, model and parameters
 * run as ONE engine call over their reads end to end, and every caller gets its own calls back in its own out[].  A launch group of 64
 * reads occupies 4 of the device's 512 tile slots for as long as one of 16 384 would (~12 ms for 4000-sample reads), so what a caller gets
 * is decided by how many calls share a group: 157 calls of 64 from one thread run one after the other (nothing to share them with; the
 * streaming entry points are the single-thread answer), from 64 threads they run as three groups.  Calls of SH_BATCH_COALESCE_MAX reads or
 * more fill the device by themselves and go straight in.  Either way the engine sees one call at a time (call_mu), which also makes this entry
 * point safe to call from several threads.  SCRAPPIE_HIP_COALESCE=0 or SCRAPPIE_HIP_BATCH_COALESCE=0: every call alone. */
#ifndef SH_BATCH_COALESCE_MAX
#define SH_BATCH_COALESCE_MAX 4096
#endif
/* (BatchReq / BatchCoalescer: scrappie_hip.hip, in front of the engine, which owns its queue -- engines of different GPUs do not wait for each other) */
static bool batch_coalesce_on() {
    static const bool on = [] { const char *v = getenv("SCRAPPIE_HIP_COALESCE"), *b = getenv("SCRAPPIE_HIP_BATCH_COALESCE"); return !(v && v[0] == '0') && !(b && b[0] == '0'); }();
    return on;
}
static int basecall_batch_direct(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out);
/* (tests, tools) engine calls the batch coalescer has made, caller calls in them, the most callers in one */
static std::atomic<unsigned long long> g_bc_batches{0}, g_bc_calls{0}, g_bc_most{0};      /* over all engines (tests, tools) */
extern "C" void scrappie_hip_batch_coalescer_stats(unsigned long long out[3]) {
    out[0] = g_bc_batches.load(); out[1] = g_bc_calls.load(); out[2] = g_bc_most.load();
}
extern "C" int scrappie_hip_basecall_batch(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n,
                                           const scrappie_hip_params *p, scrappie_hip_call *out) {
    if (!e || !reads || !out) return set_err("basecall_batch: null argument");
    if (n >= SH_BATCH_COALESCE_MAX || n == 0 || !batch_coalesce_on() || e->is_tail) {
        std::lock_guard<std::mutex> lk(e->call_mu);
        return basecall_batch_direct(e, model, reads, n, p, out);
    }
    constexpr size_t MAX_CALLS = 4096, MAX_READS = 65536;
    ShInside inside(e->batch_presence);
    BatchReq r;
    r.e = e; r.model = model; r.reads = reads; r.n = n; r.p = p ? *p : scrappie_hip_default_params(); r.out = out;
    e->batch_co.run(r, e->batch_presence, MAX_CALLS, false,
        [&](std::deque<BatchReq *> &q, std::vector<BatchReq *> &batch) {
            take_compatible(q, batch, MAX_CALLS, MAX_READS,
                            [](const BatchReq *f, const BatchReq *c) { return c->e == f->e && c->model == f->model && memcmp(&c->p, &f->p, sizeof f->p) == 0; },
                            [](const BatchReq *c) { return c->n; });
        },
        [](std::vector<BatchReq *> &) { return true; }, [](BatchReq &) {},
        [&](std::vector<BatchReq *> &batch) {
            BatchReq *f = batch[0];
            int rc;
            std::string err;
            if (batch.size() == 1) {          /* nobody to share with: the caller's own arrays */
                std::lock_guard<std::mutex> lk(f->e->call_mu);
                rc = basecall_batch_direct(f->e, f->model, f->reads, f->n, &f->p, f->out);
                if (rc) err = g_err;
            } else {
                size_t tot = 0;
                for (const BatchReq *c : batch) tot += c->n;
                std::vector<raw_table> all;
                all.reserve(tot);
                for (const BatchReq *c : batch) all.insert(all.end(), c->reads, c->reads + c->n);
                std::vector<scrappie_hip_call> calls(tot);
                {
                    std::lock_guard<std::mutex> lk(f->e->call_mu);
                    rc = basecall_batch_direct(f->e, f->model, all.data(), tot, &f->p, calls.data());
                    if (rc) err = g_err;
                }
                if (!rc) {
                    size_t at = 0;
                    for (BatchReq *c : batch) { memcpy(c->out, calls.data() + at, c->n * sizeof(scrappie_hip_call)); at += c->n; c->rc = 0; }
                } else {
                    /* the shared call failed as a whole (a failed call returns nothing): somebody's reads cannot be run -- a read too long for a launch group, say.
                     * Every caller must get what it gets ALONE, so the members run again one by one and only the one at fault fails */
                    for (BatchReq *c : batch) {
                        std::lock_guard<std::mutex> lk(f->e->call_mu);
                        c->rc = basecall_batch_direct(c->e, c->model, c->reads, c->n, &c->p, c->out);
                        c->err = c->rc ? std::string(g_err) : std::string();
                    }
                    g_bc_batches++; g_bc_calls += batch.size();
                    return;
                }
            }
            if (batch.size() == 1) { f->rc = rc; f->err = err; }
            g_bc_batches++; g_bc_calls += batch.size();
            for (unsigned long long m = g_bc_most.load(); m < batch.size() && !g_bc_most.compare_exchange_weak(m, batch.size());) { }
        });
    if (r.rc) return set_err("%s", r.err.empty() ? "basecall_batch: the shared launch failed" : r.err.c_str());
    return 0;
}
static int basecall_batch_direct(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n,
                                 const scrappie_hip_params *p, scrappie_hip_call *out) {
    Model *m = get_model(e, model);
    if (!m) return -1;
    {
        std::vector<unsigned char> is_long;
        const long nl = tail_plan(e, m, reads, n, is_long);
        if (nl < 0) return -1;
        if (nl > 0) {
            std::vector<raw_table> rl, rr;
            std::vector<size_t> il, ir;
            for (size_t i = 0; i < n; i++) { if (is_long[i]) { rl.push_back(reads[i]); il.push_back(i); } else { rr.push_back(reads[i]); ir.push_back(i); } }
            std::vector<scrappie_hip_call> orr(rr.size());
            scrappie_hip_params dp = scrappie_hip_default_params();
            auto tk = tail_submit(e, model, p ? *p : dp, std::move(rl));
            const int rc_main = basecall_batch_one(e, model, rr.data(), rr.size(), p, orr.data());
            const std::string err_main = rc_main ? std::string(g_err) : std::string();
            tail_wait(e, tk);
            (void)hipSetDevice(e->device);
            { std::lock_guard<std::mutex> lk(e->tail_mu); e->tail_open.erase(tk->id); }
            if (rc_main || tk->rc) {      /* a failed call returns nothing */
                if (!rc_main) scrappie_hip_free_calls(orr.data(), orr.size());
                if (!tk->rc) scrappie_hip_free_calls(tk->calls.data(), tk->calls.size());
                for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].basecall = nullptr; out[i].basecall_length = 0; out[i].pos = nullptr; }
                return set_err("%s", rc_main ? err_main.c_str() : tk->err.c_str());
            }
            for (size_t k = 0; k < il.size(); k++) out[il[k]] = tk->calls[k];
            for (size_t k = 0; k < ir.size(); k++) out[ir[k]] = orr[k];
            e->n_tail_calls++; e->n_tail_reads += il.size();
            return 0;
        }
    }
    return basecall_batch_one(e, model, reads, n, p, out);
}

static int basecall_batch_one(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n,
                              const scrappie_hip_params *p, scrappie_hip_call *out, scrappie_matrix *probs) {
    if (!e || !reads || !out) return set_err("basecall_batch: null argument");
    Model *m = get_model(e, model);
    if (!m) return -1;
    (void)hipSetDevice(e->device);
    const size_t per = m->arch == 3 ? (size_t)m->nfeat : 1;    /* events: lengths count events of nfeat floats */
    std::vector<uint32_t> len(n);
    for (size_t i = 0; i < n; i++) {
        const raw_table &rt = reads[i];
        const size_t ns = (rt.raw && rt.end > rt.start) ? rt.end - rt.start : 0;
        len[i] = (uint32_t)(ns / per);
    }
    std::vector<uint64_t> off[2];
    std::vector<uint32_t> glen[2];
    bool used[2] = {false, false};
    PostJob job[2];                              /* per staging slot: build_group copies it when the group is enqueued */
    return run_groups(e, model, m, len.data(), n, p, out, [&](int k, const uint32_t *idx, size_t cnt, GroupArgs &a) {
        /* staging buffer k was last read by the upload of group g-2 */
        Slot &st = e->slots[k];
        if (used[k] && e->ev_ok) HIPCHK(sh_event_wait(st.up));
        off[k].resize(cnt); glen[k].resize(cnt);
        size_t total = 0;
        for (size_t i = 0; i < cnt; i++) { glen[k][i] = len[idx[i]]; off[k][i] = total; total += (size_t)glen[k][i] * per; }
        if (st.h_sig.ensure(std::max<size_t>(total, 1) * 4) || st.d_signal.ensure(std::max<size_t>(total, 1) * 4)) return -1;
        float *hs = st.h_sig.as<float>();
        {   /* gather into the pinned staging buffer on several host threads (160 MB per 10 000 x 4000-sample group: 20 ms on one) */
            const unsigned nthr = (total * 4 > ((size_t)8 << 20)) ? std::max(1u, std::min(host_threads(), 8u)) : 1u;
            auto part = [&](size_t a, size_t b) {
                for (size_t i = a; i < b; i++)
                    if (glen[k][i]) memcpy(hs + off[k][i], reads[idx[i]].raw + reads[idx[i]].start, (size_t)glen[k][i] * per * 4);
            };
            if (nthr == 1) part(0, cnt);
            else {
                std::vector<std::thread> th;
                const size_t step = (cnt + nthr - 1) / nthr;
                for (unsigned t = 0; t < nthr; t++) { const size_t a = t * step, b = std::min(cnt, a + step); if (a < b) th.emplace_back(part, a, b); }
                for (auto &x : th) x.join();
            }
        }
        hipStream_t us = e->ev_ok ? e->ustream : e->stream;
        HIPCHK(hipMemcpyAsync(st.d_signal.p, hs, total * 4, hipMemcpyHostToDevice, us));
        if (e->ev_ok) { HIPCHK(hipEventRecord(st.up, us)); HIPCHK(hipStreamWaitEvent(e->stream, st.up, 0)); HIPCHK(hipStreamWaitEvent(e->pstream, st.up, 0)); }
        else HIPCHK(sh_stream_wait(e->stream));
        used[k] = true;
        a.d = st.d_signal.as<float>(); a.off = off[k].data(); a.len = glen[k].data();
        if (probs) {
            job[k].on = true; job[k].dst.resize(cnt);
            for (size_t i = 0; i < cnt; i++) job[k].dst[i] = probs + idx[i];
            a.pj = &job[k];
        }
        return 0;
    });
}

/* ------------------------------------------------------------------ */
/* several GPUs: reads handed out dynamically                           */
/* ------------------------------------------------------------------ */
/* The reference's one parallel axis is reads, `#pragma omp parallel for schedule(dynamic)` (scrappie_raw.c:355,387).
 * Here the unit handed out is a LAUNCH GROUP: reads are sorted by length (longest first, so the expensive groups
 * start early and the short ones fill the tail), cut into groups, and every engine's host thread takes the next
 * group from one atomic cursor when it has room for it (two groups in flight per engine).  No exchange between
 * GPUs: weights are replicated, a read lives on one GPU from signal to bases. */
extern "C" long scrappie_hip_plan_dynamic(const uint32_t *lengths, size_t n, int stride, size_t nengine, size_t max_reads,
                                          size_t max_blocks, uint32_t *order, size_t *starts, size_t cap) {
    if ((!lengths && n) || stride < 1 || nengine < 1 || max_reads < 16 || !order) return -1;
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return lengths[a] > lengths[b]; });
    memcpy(order, idx.data(), n * sizeof(uint32_t));
    /* groups small enough that every engine gets several (dynamic balance), large enough to fill a GPU:
     * about n / (4 engines) reads, between 4096 and max_reads */
    size_t per = (n + 4 * nengine - 1) / (4 * nengine);
    per = std::min(max_reads, std::max<size_t>(per, std::min<size_t>(4096, max_reads)));
    std::vector<uint32_t> sorted_len(n);
    for (size_t i = 0; i < n; i++) sorted_len[i] = lengths[idx[i]];
    return scrappie_hip_plan_groups(sorted_len.data(), n, stride, per, max_blocks, starts, cap);
}

extern "C" int scrappie_hip_basecall_batch_multi(scrappie_hip_engine *const *engines, const int *models, size_t nengine,
                                                 const raw_table *reads, size_t n, const scrappie_hip_params *p,
                                                 scrappie_hip_call *out) {
    if (!engines || !models || nengine == 0 || (!reads && n) || !out) return set_err("basecall_batch_multi: null argument");
    if (nengine == 1) return scrappie_hip_basecall_batch(engines[0], models[0], reads, n, p, out);
    scrappie_hip_params dp = scrappie_hip_default_params();
    if (!p) p = &dp;
    std::vector<Model *> ms(nengine);
    for (size_t k = 0; k < nengine; k++) {
        ms[k] = get_model(engines[k], models[k]);
        if (!ms[k]) return -1;
        if (ms[k]->stride != ms[0]->stride || ms[k]->arch != ms[0]->arch || ms[k]->NS != ms[0]->NS)
            return set_err("basecall_batch_multi: the engines hold different models");
        if (engines[k]->any_pending()) return set_err("basecall_batch_multi: launch groups are already in flight on engine %zu", k);
    }
    for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].basecall = nullptr; out[i].basecall_length = 0; out[i].pos = nullptr; }
    if (n == 0) return 0;
    const Model *m0 = ms[0];
    const size_t per = m0->arch == 3 ? (size_t)m0->nfeat : 1;
    std::vector<uint32_t> len(n), order(n);
    for (size_t i = 0; i < n; i++) {
        const raw_table &rt = reads[i];
        const size_t ns = (rt.raw && rt.end > rt.start) ? rt.end - rt.start : 0;
        len[i] = (uint32_t)(ns / per);
    }
    size_t max_reads = engines[0]->max_launch_reads, max_blocks = launch_block_cap(engines[0], ms[0]);
    for (size_t k = 1; k < nengine; k++) { max_reads = std::min(max_reads, engines[k]->max_launch_reads); max_blocks = std::min(max_blocks, launch_block_cap(engines[k], ms[k])); }
    std::vector<size_t> starts(n + 1);
    const int unit = m0->arch == 3 ? 1 : std::max(m0->stride, 1);
    const long ng = scrappie_hip_plan_dynamic(len.data(), n, unit, nengine, max_reads, max_blocks, order.data(), starts.data(), n);
    if (ng < 0) return set_err("the reads cannot be cut into launch groups (a read longer than a launch group on these devices holds, or invalid planning arguments)");
    starts.resize((size_t)ng); starts.push_back(n);

    std::atomic<long> cursor{0};
    std::atomic<int> failed{0};
    std::vector<std::string> errs(nengine);
    auto worker = [&](size_t k) {
        scrappie_hip_engine *e = engines[k];
        (void)hipSetDevice(e->device);
        struct Flight { long g = -1; std::vector<uint64_t> off; std::vector<uint32_t> len; std::vector<scrappie_hip_call> calls; };
        Flight fl[2];
        int nf = 0;                                /* groups enqueued so far on this engine */
        long prev = -1;                            /* slot index (nf - 1) & 1 holds the group not yet collected */
        auto collect_one = [&](Flight &f) -> int {
            const size_t lo = starts[(size_t)f.g], cnt = starts[(size_t)f.g + 1] - lo;
            if (scrappie_hip_collect(e, p, f.calls.data(), cnt)) return -1;
            for (size_t i = 0; i < cnt; i++) out[order[lo + i]] = f.calls[i];      /* ownership of the strings moves to out[] */
            return 0;
        };
        for (;;) {
            const long g = failed.load() ? ng : cursor.fetch_add(1);
            if (g >= ng) break;
            Flight &f = fl[nf & 1];
            const size_t lo = starts[(size_t)g], cnt = starts[(size_t)g + 1] - lo;
            Slot &st = e->slots[nf & 1];
            /* its staging buffer was last read by the upload of this engine's group nf - 2 */
            int rc = 0;
            if (nf >= 2 && e->ev_ok && sh_event_wait(st.up) != hipSuccess) rc = set_err("hipEventSynchronize failed");
            f.g = g; f.off.resize(cnt); f.len.resize(cnt); f.calls.assign(cnt, scrappie_hip_call{});
            size_t total = 0;
            for (size_t i = 0; i < cnt; i++) { f.len[i] = len[order[lo + i]]; f.off[i] = total; total += (size_t)f.len[i] * per; }
            if (!rc && (st.h_sig.ensure(std::max<size_t>(total, 1) * 4) || st.d_signal.ensure(std::max<size_t>(total, 1) * 4))) rc = -1;
            if (!rc) {
                float *hs = st.h_sig.as<float>();
                for (size_t i = 0; i < cnt; i++) {
                    const raw_table &rt = reads[order[lo + i]];
                    if (f.len[i]) memcpy(hs + f.off[i], rt.raw + rt.start, (size_t)f.len[i] * per * 4);
                }
                hipStream_t us = e->ev_ok ? e->ustream : e->stream;
                if (hipMemcpyAsync(st.d_signal.p, hs, total * 4, hipMemcpyHostToDevice, us) != hipSuccess) rc = set_err("hipMemcpyAsync (signals) failed");
                if (!rc && e->ev_ok && (hipEventRecord(st.up, us) != hipSuccess || hipStreamWaitEvent(e->stream, st.up, 0) != hipSuccess || hipStreamWaitEvent(e->pstream, st.up, 0) != hipSuccess)) rc = set_err("event failed");
                if (!rc && !e->ev_ok && sh_stream_wait(e->stream) != hipSuccess) rc = set_err("sync failed");
            }
            if (!rc && scrappie_hip_run_device(e, models[k], st.d_signal.as<float>(), f.off.data(), f.len.data(), cnt, p) < 0) rc = -1;
            if (!rc) nf++;
            if (!rc && prev >= 0 && collect_one(fl[(nf - 2) & 1])) rc = -1;      /* the older group, while the new one runs */
            if (rc) { errs[k] = scrappie_hip_last_error(); failed.store(1); break; }
            prev = g;
        }
        if (!failed.load() && prev >= 0 && collect_one(fl[(nf - 1) & 1])) { errs[k] = scrappie_hip_last_error(); failed.store(1); }
        if (failed.load()) e->drain();
    };
    /* the engines of one call share the host: each stitches with its share of the CPUs this process may use */
    for (size_t k = 0; k < nengine; k++) engines[k]->host_thread_budget = std::max(1u, host_threads() / (unsigned)nengine);
    std::vector<std::thread> th;
    for (size_t k = 0; k < nengine; k++) th.emplace_back(worker, k);
    for (auto &t : th) t.join();
    for (size_t k = 0; k < nengine; k++) engines[k]->host_thread_budget = 0;
    if (failed.load()) {
        /* out[] owns the strings of every launch group collected before the failure: a failed call returns nothing,
         * so they are released here and out[] is left as it would be for n reads without a call */
        scrappie_hip_free_calls(out, n);
        for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].basecall = nullptr; out[i].basecall_length = 0; out[i].pos = nullptr; }
        for (size_t k = 0; k < nengine; k++) if (!errs[k].empty()) return set_err("engine %zu: %s", k, errs[k].c_str());
        return set_err("basecall_batch_multi failed");
    }
    return 0;
}
