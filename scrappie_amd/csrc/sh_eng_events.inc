/* sh_eng_events.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * event detection (sh_events.h).  scrappie_hip_detect_events_batch sorts a call's reads by length (a wave of the serial kernels holds
 * 64 reads and lasts as long as its longest), cuts them into launches under a slot budget (LaunchCut, sh_eng_cut.inc) and runs each
 * launch as signals up -> k_ev_sums -> k_ev_tstat -> k_ev_peaks -> peak counts back -> k_ev_events -> event tables back.  The
 * reference's detect_events is a batch of one on the process-default engine.  At the end: scrappie_hip_basecall_events_batch, `scrappie events`
 * for a batch, with the stitching in dwell mode (sh_dwell.h). */

/* host side of one launch: the reads' records in device order (who[] of the cutter says whose) */
struct EvPlan {
    std::vector<ShEvRead> rd;
    long long samples = 0, slots = 0;
};

static void ev_plan_add(EvPlan &pl, size_t nsample) {
    ShEvRead r{};
    r.n = (int)nsample;
    r.sig = pl.samples; pl.samples += (long long)nsample;
    r.slot = pl.slots; pl.slots += (long long)nsample + 1;
    pl.rd.push_back(r);
}

extern "C" long long scrappie_hip_events_plan_scratch(const size_t *nsample, size_t n, long long *off) {
    EvPlan pl;
    for (size_t i = 0; i < n; i++) {
        ev_plan_add(pl, nsample[i]);
        if (off) off[i] = pl.rd[i].slot;
    }
    return pl.slots;
}

/* the call's reads sorted by length, longest first (stable: equal lengths keep their input order), as run_groups sorts a basecall's */
static void ev_length_order(const size_t *nsample, size_t n, std::vector<uint32_t> &order) {
    order.resize(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return nsample[a] > nsample[b]; });
}

extern "C" long scrappie_hip_events_plan_launches(const size_t *nsample, size_t n, size_t budget_slots, uint32_t *order, size_t *starts, size_t cap) {
    if ((!nsample && n) || budget_slots < 1) return -1;
    std::vector<uint32_t> ord;
    ev_length_order(nsample, n, ord);
    long ng = 0;
    size_t used = 0, cnt = 0;
    for (size_t k = 0; k < n; k++) {
        const size_t need = nsample[ord[k]] + 1;
        if (need > budget_slots) return -1;
        if (cnt == 0 || used + need > budget_slots) {
            if (starts && (size_t)ng < cap) starts[ng] = k;
            ng++; used = 0; cnt = 0;
        }
        used += need; cnt++;
        if (order) order[k] = ord[k];
    }
    return ng;
}

static std::atomic<uint64_t> g_event_launches;
extern "C" uint64_t scrappie_hip_event_launch_count(void) { return g_event_launches.load(std::memory_order_relaxed); }
extern "C" size_t scrappie_hip_event_tile(void) { return SH_EV_TILE; }
extern "C" void scrappie_hip_event_timing(scrappie_hip_engine *e, double out[3]) { timing3(e ? e->event_ms : nullptr, out); }

extern "C" void scrappie_hip_free_event_results(scrappie_hip_event_result *r, size_t n) {
    if (!r) return;
    for (size_t i = 0; i < n; i++) { free(r[i].events.event); r[i].events = event_table{0, 0, 0, nullptr}; }
}

/* device bytes of a launch besides its event tables, per slot: 28 of scratch, the signal, and the same again in pinned staging is the host's */
static constexpr size_t EV_SLOT_BYTES = 28 + 4;

/* one launch over the reads who[] of the call (already in length order): out[who] gets its event table, or status 1 */
static int ev_run(scrappie_hip_engine *e, const std::vector<size_t> &who, EvPlan &pl, const raw_table *reads, const ShEvParams &prm,
                  scrappie_hip_event_result *out) {
    const size_t n = pl.rd.size();
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nslot = (size_t)pl.slots, nsamp = (size_t)pl.samples;
    /* checked reservations: the five scratch arrays, signals, records, counts and offsets; pinned: signals | records, later counts | offsets | tables */
    if (e->d_ev_sum.ensure(nslot * 8) || e->d_ev_sumsq.ensure(nslot * 8) || e->d_ev_t1.ensure(nslot * 4) || e->d_ev_t2.ensure(nslot * 4) ||
        e->d_ev_peaks.ensure(nslot * 4) || e->d_ev_sig.ensure(nsamp * 4 + 16) || e->d_ev_rd.ensure(n * sizeof(ShEvRead)) ||
        e->d_ev_np.ensure(n * 4) || e->d_ev_off.ensure((n + 1) * 8)) return -1;
    const size_t sig_bytes = (nsamp * 4 + 15) & ~(size_t)15;
    if (e->h_ev.ensure(sig_bytes + n * sizeof(ShEvRead) + n * 4 + (n + 1) * 8 + 64)) return -1;
    float *hsig = e->h_ev.as<float>();
    ShEvRead *hrd = (ShEvRead *)(e->h_ev.as<char>() + sig_bytes);
    long long *hoff = (long long *)(hrd + n);
    int *hnp = (int *)(hoff + n + 1);
    for (size_t k = 0; k < n; k++) {
        const raw_table &rt = reads[who[k]];
        memcpy(hsig + pl.rd[k].sig, rt.raw + rt.start, (size_t)pl.rd[k].n * 4);
        hrd[k] = pl.rd[k];
    }
    HIPCHK(hipMemcpyAsync(e->d_ev_sig.p, hsig, nsamp * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_ev_rd.p, hrd, n * sizeof(ShEvRead), hipMemcpyHostToDevice, s));
    HIPCHK(sh_stream_wait(s));
    const auto t1 = std::chrono::steady_clock::now();
    const ShEvRead *rd = e->d_ev_rd.as<ShEvRead>();
    double *sum = e->d_ev_sum.as<double>(), *sumsq = e->d_ev_sumsq.as<double>();
    float *ts1 = e->d_ev_t1.as<float>(), *ts2 = e->d_ev_t2.as<float>();
    unsigned *peaks = e->d_ev_peaks.as<unsigned>();
    int *np = e->d_ev_np.as<int>();
    const dim3 waves((unsigned)((n + SH_EV_READS - 1) / SH_EV_READS)), per_slot((unsigned)((nslot + 255) / 256));
    g_event_launches.fetch_add(1, std::memory_order_relaxed);
    if (launch_k<k_ev_sums>(waves, dim3(SH_EV_READS), 0, s, rd, (int)n, (const float *)e->d_ev_sig.as<float>(), sum, sumsq) ||
        launch_k<k_ev_tstat>(per_slot, dim3(256), 0, s, rd, (int)n, (long long)nslot, (const double *)sum, (const double *)sumsq, ts1, ts2, prm) ||
        launch_k<k_ev_peaks>(waves, dim3(SH_EV_READS), 0, s, rd, (int)n, (const float *)ts1, (const float *)ts2, peaks, np, prm)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hnp, np, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    /* a read with peaks has one event more than peaks; one without has no table */
    long long nev = 0;
    for (size_t k = 0; k < n; k++) { hoff[k] = nev; nev += hnp[k] > 0 ? (long long)hnp[k] + 1 : 0; }
    hoff[n] = nev;
    event_t *hev = nullptr;
    auto t3 = std::chrono::steady_clock::now();      /* the kernels are over: here, or behind k_ev_events */
    if (nev > 0) {
        if (e->d_ev_out.ensure((size_t)nev * sizeof(event_t)) || e->h_ev_out.ensure((size_t)nev * sizeof(event_t))) return -1;
        HIPCHK(hipMemcpyAsync(e->d_ev_off.p, hoff, (n + 1) * 8, hipMemcpyHostToDevice, s));
        if (launch_k<k_ev_events>(dim3((unsigned)((nev + 255) / 256)), dim3(256), 0, s, rd, (int)n, (const long long *)e->d_ev_off.as<long long>(), (const double *)sum,
                                  (const double *)sumsq, (const unsigned *)peaks, e->d_ev_out.as<uint4>())) return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(sh_stream_wait(s));
        t3 = std::chrono::steady_clock::now();
        hev = e->h_ev_out.as<event_t>();
        HIPCHK(hipMemcpyAsync(hev, e->d_ev_out.p, (size_t)nev * sizeof(event_t), hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
    }
    for (size_t k = 0; k < n; k++) {
        scrappie_hip_event_result &res = out[who[k]];
        const size_t m = (size_t)(hoff[k + 1] - hoff[k]);
        if (m == 0) { res.status = 1; continue; }
        res.events.event = (event_t *)malloc(m * sizeof(event_t));
        if (!res.events.event) return set_err("out of host memory");
        memcpy(res.events.event, hev + hoff[k], m * sizeof(event_t));
        res.events.n = m; res.events.start = 0; res.events.end = m;
        res.status = 0;
    }
    const auto t4 = std::chrono::steady_clock::now();
    e->event_ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    e->event_ms[1] += std::chrono::duration<double, std::milli>(t3 - t1).count();
    e->event_ms[2] += std::chrono::duration<double, std::milli>(t4 - t3).count();
    return 0;
}

static int ev_read_ok(const char *fn, const raw_table &rt) {
    if (!rt.raw) return set_err("%s: no signal", fn);
    if (rt.start >= rt.end) return set_err("%s: an empty signal window [%zu, %zu)", fn, rt.start, rt.end);
    if (rt.end > rt.n) return set_err("%s: the signal window ends at %zu, past its %zu samples", fn, rt.end, rt.n);
    if (rt.end - rt.start > (size_t)INT32_MAX / 2) return set_err("%s: %zu samples is too many", fn, rt.end - rt.start);
    return 0;
}

static int ev_params(const char *fn, const detector_param *p, ShEvParams &prm) {
    const detector_param d = p ? *p : event_detection_defaults;
    if (d.window_length1 > SH_EV_MAX_WINDOW || d.window_length2 > SH_EV_MAX_WINDOW)
        return set_err("%s: windows of %zu and %zu samples (at most %d)", fn, d.window_length1, d.window_length2, SH_EV_MAX_WINDOW);
    prm.w1 = (int)d.window_length1; prm.w2 = (int)d.window_length2;
    prm.threshold1 = d.threshold1; prm.threshold2 = d.threshold2; prm.peak_height = d.peak_height;
    return 0;
}

extern "C" int scrappie_hip_detect_events_batch(scrappie_hip_engine *e, const raw_table *reads, size_t n, const detector_param *p,
                                                scrappie_hip_event_result *results) {
    if (!e || (n && (!reads || !results))) return set_err("detect_events_batch: null argument");
    for (size_t i = 0; i < n; i++) { results[i].events = event_table{0, 0, 0, nullptr}; results[i].status = 2; }
    ShEvParams prm{};
    if (ev_params("detect_events_batch", p, prm)) return -1;
    (void)hipSetDevice(e->device);
    { std::lock_guard<std::mutex> lk(e->mu); for (double &x : e->event_ms) x = 0.0; }
    const size_t budget = e->dbg_events_budget ? e->dbg_events_budget : std::max<size_t>(launch_budget(e, 0) / (EV_SLOT_BYTES + sizeof(event_t)), 1);
    std::vector<size_t> ns(n);
    for (size_t i = 0; i < n; i++) ns[i] = (reads[i].raw && reads[i].end > reads[i].start) ? reads[i].end - reads[i].start : 0;
    std::vector<uint32_t> order;
    ev_length_order(ns.data(), n, order);
    LaunchCut<EvPlan> cut{e, "detect_events_batch"};
    cut.run = [&](const std::vector<size_t> &who, EvPlan &pl) { return ev_run(e, who, pl, reads, prm, results); };
    for (size_t k = 0; k < n && !cut.failed; k++) {
        const size_t i = order[k];
        if (ev_read_ok("detect_events_batch", reads[i])) { cut.refuse(i, g_err); continue; }
        if (ns[i] + 1 > budget) {
            char msg[160];
            snprintf(msg, sizeof msg, "detect_events_batch: %zu samples are more than one launch may hold (%zu slots)", ns[i], budget);
            cut.refuse(i, msg);
            continue;
        }
        cut.add(i, (size_t)cut.load.slots + ns[i] + 1 <= budget && cut.who.size() < (size_t)INT32_MAX / 2);
        ev_plan_add(cut.load, ns[i]);
    }
    return cut.finish([&] { scrappie_hip_free_event_results(results, n); for (size_t i = 0; i < n; i++) results[i].status = 2; },
                      [](size_t i, const char *why) { set_err("%s (read %zu of the call)", why, i); });
}

/* ------------------------------------------------------------------ */
/* per-read reference surface (event_detection.c:268)                   */
/* ------------------------------------------------------------------ */
extern "C" event_table detect_events(raw_table const rt, detector_param const edparam) {
    const event_table none{0, 0, 0, nullptr};
    if (ev_read_ok("detect_events", rt)) return none;                     /* RETURN_NULL_IF(NULL == rt.raw, et), and the windows the reference asserts on */
    scrappie_hip_engine *e = default_engine();
    if (!e) return none;
    scrappie_hip_event_result res;
    if (scrappie_hip_detect_events_batch(e, &rt, 1, &edparam, &res)) return none;
    if (res.status == 1) set_err("detect_events: no peak in %zu samples, so no event table (the reference is undefined there)", rt.end - rt.start);
    return res.events;
}

/* ------------------------------------------------------------------ */
/* `scrappie events` for a batch (scrappie_events.c:271-330)            */
/* ------------------------------------------------------------------ */
/* Detection (batched, above) -> features on host threads (sh_host.c; they stay there: the reference studentises with rsqrtps, whose bits are the
 * CPU's own) -> the events model's launch groups, as scrappie_hip_basecall_batch cuts them, with the stitching in dwell mode (sh_dwell.h) when
 * asked.  A group's dwells -- (int)event.length, 4 bytes an event -- ride behind its feature matrices (48 bytes an event) in the same staging
 * buffer and the same upload; the group's DwellJob (GroupArgs) says where, in the order the length sort and the cut have given the group. */
extern "C" int scrappie_hip_basecall_events_batch(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n, const detector_param *dp,
                                                  const scrappie_hip_params *params, int dwell_correction, scrappie_hip_call *out) {
    if (!e || (n && (!reads || !out))) return set_err("basecall_events_batch: null argument");
    Model *m = get_model(e, model);
    if (!m) return -1;
    if (m->arch != 3) return set_err("basecall_events_batch: the model is not an events model");
    for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].basecall = nullptr; out[i].basecall_length = 0; out[i].pos = nullptr; }
    if (n == 0) return 0;
    std::vector<scrappie_hip_event_result> evs(n);
    if (scrappie_hip_detect_events_batch(e, reads, n, dp, evs.data())) return -1;
    struct FreeEvents { std::vector<scrappie_hip_event_result> &v; ~FreeEvents() { scrappie_hip_free_event_results(v.data(), v.size()); } } free_events{evs};
    const size_t per = (size_t)m->nfeat;
    std::vector<size_t> keep, at;      /* the reads with an event table, and where each one's events begin in the flat arrays */
    size_t nev = 0;
    for (size_t i = 0; i < n; i++) {
        if (!evs[i].events.event || evs[i].events.n == 0) continue;
        if (evs[i].events.n > (size_t)INT32_MAX / 16) return set_err("basecall_events_batch: %zu events in read %zu", evs[i].events.n, i);
        keep.push_back(i); at.push_back(nev); nev += evs[i].events.n;
    }
    const size_t nk = keep.size();
    if (nk == 0) return 0;
    std::vector<float> feat(nev * per), num(nk);
    std::vector<int> dwell(dwell_correction ? nev : 0);
    std::vector<uint32_t> len(nk);
    std::atomic<int> feat_failed{0};
    {
        auto part = [&](size_t a, size_t b) {
            for (size_t k = a; k < b; k++) {
                const event_table &et = evs[keep[k]].events;
                len[k] = (uint32_t)et.n;
                if (scrappie_hip_event_features(et, feat.data() + at[k] * per)) feat_failed.store(1);
                num[k] = sh_dwell_prior_num(et.event, et.n);
                if (dwell_correction) for (size_t j = 0; j < et.n; j++) dwell[at[k] + j] = (int)et.event[j].length;
            }
        };
        const unsigned nthr = nev > 65536 ? std::max(1u, std::min(host_threads(), 16u)) : 1u;
        if (nthr == 1) part(0, nk);
        else {
            std::vector<std::thread> th;
            const size_t step = (nk + nthr - 1) / nthr;
            for (unsigned t = 0; t < nthr; t++) { const size_t a = t * step, b = std::min(nk, a + step); if (a < b) th.emplace_back(part, a, b); }
            for (auto &x : th) x.join();
        }
    }
    if (feat_failed.load()) return set_err("basecall_events_batch: event features failed");
    scrappie_hip_params pp = params ? *params : scrappie_hip_default_params();
    pp.homopolymer = 0;                          /* the posterior-mean homopolymer pass is `scrappie raw`'s */
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->call_mu);
    DwellJob job[2];                             /* per staging slot: build_group copies it when the group is enqueued */
    std::vector<uint64_t> off[2];
    std::vector<uint32_t> glen[2];
    bool used[2] = {false, false};
    return run_groups(e, model, m, len.data(), nk, &pp, out, [&](int k, const uint32_t *idx, size_t cnt, GroupArgs &a) {
        Slot &st = e->slots[k];
        if (used[k] && e->ev_ok) HIPCHK(sh_event_wait(st.up));      /* staging buffer k was last read by the upload of group g-2 */
        off[k].resize(cnt); glen[k].resize(cnt);
        size_t total = 0, gev = 0;
        for (size_t i = 0; i < cnt; i++) { glen[k][i] = len[idx[i]]; off[k][i] = total; total += (size_t)glen[k][i] * per; gev += glen[k][i]; }
        const size_t words = total + (dwell_correction ? gev : 0);
        if (st.h_sig.ensure(std::max<size_t>(words, 1) * 4) || st.d_signal.ensure(std::max<size_t>(words, 1) * 4)) return -1;
        float *hs = st.h_sig.as<float>();
        for (size_t i = 0; i < cnt; i++) memcpy(hs + off[k][i], feat.data() + at[idx[i]] * per, (size_t)glen[k][i] * per * 4);
        if (dwell_correction) {
            int *hd = (int *)(hs + total);
            DwellJob &j = job[k];
            j.on = true; j.d_dwell = (const int *)(st.d_signal.as<float>() + total);
            j.off.resize(cnt); j.num.resize(cnt); j.host.resize(cnt);
            size_t w = 0;
            for (size_t i = 0; i < cnt; i++) {
                const int *src = dwell.data() + at[idx[i]];
                memcpy(hd + w, src, (size_t)glen[k][i] * 4);
                j.off[i] = w; j.num[i] = num[idx[i]]; j.host[i] = src;
                w += glen[k][i];
            }
        }
        hipStream_t us = e->ev_ok ? e->ustream : e->stream;
        HIPCHK(hipMemcpyAsync(st.d_signal.p, hs, words * 4, hipMemcpyHostToDevice, us));
        if (e->ev_ok) { HIPCHK(hipEventRecord(st.up, us)); HIPCHK(hipStreamWaitEvent(e->stream, st.up, 0)); HIPCHK(hipStreamWaitEvent(e->pstream, st.up, 0)); }
        else HIPCHK(sh_stream_wait(e->stream));
        used[k] = true;
        a.d = st.d_signal.as<float>(); a.off = off[k].data(); a.len = glen[k].data(); a.dw = dwell_correction ? &job[k] : nullptr;
        return 0;
    }, false, keep.data());
}
