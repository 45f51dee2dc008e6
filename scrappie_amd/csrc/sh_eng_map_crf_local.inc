/* sh_eng_map_crf_local.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * reads of a flip-flop (CRF) model mapped INTO a longer base sequence (k_map_crf_local, sh_map_crf_local.h).  Two passes, as
 * sh_eng_map_pack.inc: every window of every read of a launch in ONE k_map_crf_local launch (per home), scores and end cells back, the
 * host picks each read's best window (or sums them); with a path wanted a second launch runs the traceback on that window alone
 * and k_map_crf_local_walk returns path and first.  map_crf_to_reference_* on the process-default engine (the caller's host matrix
 * uploaded, the reference-layout loader) and scrappie_hip_map_local_batch: the network and k_crf<true> of a launch group
 * (run_staged to STOP_POST), both passes on the transitions where k_crf left them in d_E, under the engine's lock.  The cut of a
 * sequence into windows is host arithmetic in sh_host.c (scrappie_hip_map_crf_local_plan). */

/* launches of each k_map_crf_local form in this process: index (vit ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_map_crf_local_forms[8];
extern "C" void scrappie_hip_map_crf_local_form_counts(uint64_t forms[8]) {
    if (forms) for (int i = 0; i < 8; i++) forms[i] = g_map_crf_local_forms[i].load(std::memory_order_relaxed);
}

static const size_t MAP_LOCAL_MAX_SEQ = (size_t)1 << 30;      /* a cell and its kind share an int32 */

/* one read of a launch: where its transitions are (as map_crf_plan_add takes them), its sequence, and what comes back */
struct MapLocalJob {
    long long trans; int lane; size_t nblock;
    const int *seq; size_t L;
    float score = NAN; size_t first = (size_t)-1, last = 0; int32_t *path = nullptr;
};

/* the windows of a sequence for a read, as the planner cuts them */
struct MapLocalCut { std::vector<size_t> first, ncell, own; std::vector<int> home; std::vector<long long> scr; };
static long long map_local_cut(size_t L, size_t nblock, long stride, MapLocalCut *c) {
    const long long nw = scrappie_hip_map_crf_local_plan(L, nblock, stride, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!c || nw <= 0) return nw;
    const size_t n = (size_t)nw;
    c->first.resize(n); c->ncell.resize(n); c->own.resize(n); c->home.resize(n); c->scr.resize(n);
    long long fl = 0;
    return scrappie_hip_map_crf_local_plan(L, nblock, stride, n, c->first.data(), c->ncell.data(), c->own.data(), c->home.data(), c->scr.data(), &fl);
}

static long long map_local_tb_words(size_t ncell, size_t nblock) { return (long long)nblock * (long long)(4 * ((ncell + 63) / 64)); }

/* device bytes one read adds to a launch, its sequence apart: the first pass's windows, scores, end cells and scratch rows; with a
 * path the second pass's traceback and rows on its largest window, and the path */
static size_t map_local_read_bytes(size_t L, size_t nblock, long stride, bool path) {
    long long fl = 0;
    const long long nw = scrappie_hip_map_crf_local_plan(L, nblock, stride, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &fl);
    size_t b = (size_t)nw * (sizeof(ShMapCrfLocalWin) + 12) + (size_t)fl * 4 + 64;
    if (path) {
        const size_t s = scrappie_hip_map_crf_local_stride(L, nblock, stride);
        const size_t nc = std::min(s + nblock, L + 1);
        b += (size_t)map_local_tb_words(nc, nblock) * 4 + (nblock + 1) * 4 + 4 * (nc + 1) * 4 + sizeof(ShMapCrfLocalWin) + 64;
    }
    return b;
}

/* util.h:162-164 on the host: the windows' forward scores, in window order */
static float map_local_lse(float x, float y) { return fmaxf(x, y) + log1pf(expf(-fabsf(x - y))); }

/* one launch of windows rd[] (those of the LDS home first: n_lds of them) through k_map_crf_local; scores and, Viterbi, end cells
 * into h_mcl ([n] float, then [n] int2) */
static int map_local_launch(scrappie_hip_engine *e, const std::vector<ShMapCrfLocalWin> &rd, size_t n_lds, size_t lds, long long scr_floats, long long tb_words,
                            const float *trans, bool vit, bool tiled) {
    hipStream_t s = e->stream;
    const size_t n = rd.size();
    if (e->d_mcl_rd.ensure(n * sizeof(ShMapCrfLocalWin)) || e->d_mcl_scr.ensure((size_t)scr_floats * 4 + 16) || e->d_mcl_score.ensure(n * 4 + 16) ||
        e->d_mcl_end.ensure(n * 8 + 16) || e->d_mcl_tb.ensure((size_t)tb_words * 4 + 16) || e->h_mcl.ensure(n * 12 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(e->d_mcl_rd.p, rd.data(), n * sizeof(ShMapCrfLocalWin), hipMemcpyHostToDevice, s));
    ShMapCrfLocalArgs a{};
    a.rd = e->d_mcl_rd.as<ShMapCrfLocalWin>(); a.trans = trans; a.seq = e->d_mcl_seq.as<int>(); a.tb = e->d_mcl_tb.as<unsigned>();
    a.scr = e->d_mcl_scr.as<float>(); a.score = e->d_mcl_score.as<float>(); a.final_state = e->d_mcl_end.as<int2>();
    if (lds > SH_MAP_LDS) return set_err("map_crf_local: a window of %zu bytes of LDS", lds);
    if (pick_bool([&](auto v, auto tl) {
            using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
            return dp_launch<k_map_crf_local<v(), LD, true>, k_map_crf_local<v(), LD, false>>(s, a, n_lds, n, SH_MAP_NTH, lds, SH_MAPC_HEAD * 4,
                                                                                             g_map_crf_local_forms + ((v() ? 4 : 0) | (tl() ? 2 : 0)));
        }, vit, tiled)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->h_mcl.p, e->d_mcl_score.p, n * 4, hipMemcpyDeviceToHost, s));
    if (vit) HIPCHK(hipMemcpyAsync((char *)e->h_mcl.p + n * 4, e->d_mcl_end.p, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    return 0;
}

/* Both passes over jobs[] (under mu).  trans: d_E or the uploaded matrices.  A sequence several jobs point at is uploaded once.
 * want_first: the second pass (path and first) on each job's best window.  t (may be NULL): t[0] += the first pass, t[1] += the
 * second pass, the walk and the copies. */
static int map_local_run(scrappie_hip_engine *e, std::vector<MapLocalJob> &jobs, const float *trans, bool vit, bool tiled, bool want_first, double *t) {
    const size_t nj = jobs.size();
    if (nj == 0) return 0;
    hipStream_t s = e->stream;
    const long stride = (long)e->map_crf_local_stride;
    const auto t0 = std::chrono::steady_clock::now();
    /* the sequences, each once */
    std::map<std::pair<const int *, size_t>, long long> at;
    long long ncode = 0;
    for (const MapLocalJob &j : jobs)
        if (at.emplace(std::make_pair(j.seq, j.L), ncode).second) ncode += (long long)j.L;
    if (e->d_mcl_seq.ensure((size_t)ncode * 4 + 16)) return -1;
    for (const auto &kv : at)
        HIPCHK(hipMemcpyAsync((char *)e->d_mcl_seq.p + (size_t)kv.second * 4, kv.first.first, kv.first.second * 4, hipMemcpyHostToDevice, s));
    /* the windows: those of the LDS home first, each home in job and window order */
    std::vector<ShMapCrfLocalWin> rd[2];
    std::vector<size_t> slot[2];               /* where a window's score goes: job_off[job] + w */
    std::vector<size_t> job_off(nj + 1, 0);
    std::map<std::pair<size_t, size_t>, MapLocalCut> cut_of;      /* (bases, blocks): reads of one length share a sequence's cut */
    std::vector<const MapLocalCut *> cuts(nj, nullptr);
    long long scr_floats = 0;
    size_t lds = 0;
    for (size_t k = 0; k < nj; k++) {
        const MapLocalJob &j = jobs[k];
        auto found = cut_of.find(std::make_pair(j.L, j.nblock));
        if (found == cut_of.end()) {
            found = cut_of.emplace(std::make_pair(j.L, j.nblock), MapLocalCut()).first;
            (void)map_local_cut(j.L, j.nblock, stride, &found->second);
        }
        cuts[k] = &found->second;
        const long long nw = (long long)found->second.first.size();
        if (nw <= 0) return set_err("map_crf_local: nothing to cut (a sequence of %zu bases, %zu blocks)", j.L, j.nblock);
        job_off[k + 1] = job_off[k] + (size_t)nw;
        for (size_t w = 0; w < (size_t)nw; w++) {
            const MapLocalCut &c = *cuts[k];
            ShMapCrfLocalWin r{};
            r.trans = j.trans; r.lane = j.lane; r.nblock = (int)j.nblock; r.seqlen = (int)j.L; r.seq = at[std::make_pair(j.seq, j.L)];
            r.first = (int)c.first[w]; r.ncell = (int)c.ncell[w]; r.own = (int)c.own[w]; r.ok = 1; r.tb = -1;
            const int h = c.home[w];
            if (h) { r.scr = scr_floats; scr_floats += (long long)(4 * (c.ncell[w] + 1)); }
            else { r.scr = -1; lds = std::max(lds, sh_map_crf_local_lds_bytes(c.ncell[w])); }
            rd[h].push_back(r);
            slot[h].push_back(job_off[k] + w);
        }
    }
    const size_t n_lds = rd[0].size(), nwin = job_off[nj];
    rd[0].insert(rd[0].end(), rd[1].begin(), rd[1].end());
    slot[0].insert(slot[0].end(), slot[1].begin(), slot[1].end());
    if (map_local_launch(e, rd[0], n_lds, lds, scr_floats, 0, trans, vit, tiled)) return -1;
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<float> wsc(nwin);
    std::vector<int2> wend(vit ? nwin : 0);
    {
        const float *hs = e->h_mcl.as<float>();
        const int2 *he = (const int2 *)(hs + nwin);
        for (size_t k = 0; k < nwin; k++) { wsc[slot[0][k]] = hs[k]; if (vit) wend[slot[0][k]] = he[k]; }
    }
    /* per read: the highest window, the lowest on a tie; forward: sh_lse over the windows in their order */
    std::vector<size_t> bestw(nj, 0);
    for (size_t k = 0; k < nj; k++) {
        const float *sc = wsc.data() + job_off[k];
        const size_t nw = job_off[k + 1] - job_off[k];
        MapLocalJob &j = jobs[k];
        if (vit) {
            size_t b = 0;
            for (size_t w = 1; w < nw; w++) if (sc[w] > sc[b]) b = w;
            bestw[k] = b;
            j.score = sc[b];
            j.last = (size_t)wend[job_off[k] + b].x;
        } else {
            float acc = sc[0];
            for (size_t w = 1; w < nw; w++) acc = map_local_lse(acc, sc[w]);
            j.score = acc;
        }
    }
    if (vit && want_first) {
        /* the second pass: each read's best window alone, with its traceback */
        std::vector<ShMapCrfLocalWin> r2[2];
        std::vector<size_t> who[2];
        long long tb_words = 0, scr2 = 0, path_len = 0;
        size_t lds2 = 0;
        for (size_t k = 0; k < nj; k++) {
            const MapLocalJob &j = jobs[k];
            const MapLocalCut &c = *cuts[k];
            const size_t w = bestw[k];
            ShMapCrfLocalWin r{};
            r.trans = j.trans; r.lane = j.lane; r.nblock = (int)j.nblock; r.seqlen = (int)j.L; r.seq = at[std::make_pair(j.seq, j.L)];
            r.first = (int)c.first[w]; r.ncell = (int)c.ncell[w]; r.own = (int)c.own[w]; r.ok = 1;
            r.tb = tb_words; tb_words += map_local_tb_words(c.ncell[w], j.nblock);
            const int h = c.home[w];
            if (h) { r.scr = scr2; scr2 += (long long)(4 * (c.ncell[w] + 1)); }
            else { r.scr = -1; lds2 = std::max(lds2, sh_map_crf_local_lds_bytes(c.ncell[w])); }
            r2[h].push_back(r);
            who[h].push_back(k);
        }
        const size_t n2_lds = r2[0].size();
        r2[0].insert(r2[0].end(), r2[1].begin(), r2[1].end());
        who[0].insert(who[0].end(), who[1].begin(), who[1].end());
        std::vector<long long> poff(nj);
        for (size_t k = 0; k < nj; k++) { poff[k] = path_len; path_len += (long long)jobs[who[0][k]].nblock + 1; }
        if (map_local_launch(e, r2[0], n2_lds, lds2, scr2, tb_words, trans, true, tiled)) return -1;
        {
            const float *hs = e->h_mcl.as<float>();          /* the same window again: the same bits */
            const int2 *he = (const int2 *)(hs + nj);
            for (size_t k = 0; k < nj; k++) {
                const MapLocalJob &j = jobs[who[0][k]];
                if (memcmp(&hs[k], &j.score, 4) || (size_t)he[k].x != j.last)
                    return set_err("map_crf_local: the second pass of a window disagrees with the first (%.9g at %d, not %.9g at %zu)", hs[k], he[k].x, j.score, j.last);
            }
        }
        if (e->d_mcl_poff.ensure(nj * 8) || e->d_mcl_path.ensure((size_t)path_len * 4 + 16) || e->d_mcl_first.ensure(nj * 4 + 16) ||
            e->h_mcl.ensure(nj * 16 + (size_t)path_len * 4 + 16)) return -1;
        HIPCHK(hipMemcpyAsync(e->d_mcl_poff.p, poff.data(), nj * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_map_crf_local_walk, dim3((unsigned)((nj + 63) / 64)), dim3(64), 0, s, (const ShMapCrfLocalWin *)e->d_mcl_rd.p, (int)nj,
                           (const unsigned *)e->d_mcl_tb.p, (const int2 *)e->d_mcl_end.p, (const long long *)e->d_mcl_poff.p, e->d_mcl_path.as<int>(),
                           e->d_mcl_first.as<int>());
        HIPCHK(hipGetLastError());
        int32_t *hf = (int32_t *)e->h_mcl.p, *hp = hf + nj;
        HIPCHK(hipMemcpyAsync(hf, e->d_mcl_first.p, nj * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hp, e->d_mcl_path.p, (size_t)path_len * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
        for (size_t k = 0; k < nj; k++) {
            MapLocalJob &j = jobs[who[0][k]];
            j.first = (size_t)hf[k];
            j.path = (int32_t *)malloc((j.nblock + 1) * 4);
            if (!j.path) return set_err("out of host memory");
            memcpy(j.path, hp + poff[k], (j.nblock + 1) * 4);
        }
    }
    if (t) {
        t[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    return 0;
}

/* the checks a sequence passes before it reaches the kernel; 0 or -1 with the reason */
static int map_local_target_ok(const char *fn, const int *seq, size_t L) {
    if (!seq) return set_err("%s: no sequence", fn);
    if (L == 0) return set_err("%s: an empty sequence", fn);
    if (L > MAP_LOCAL_MAX_SEQ) return set_err("%s: a sequence of %zu bases is longer than the %zu a cell index holds", fn, L, MAP_LOCAL_MAX_SEQ);
    for (size_t i = 0; i < L; i++)
        if (seq[i] < 0 || seq[i] > 3) return set_err("%s: sequence code %d at %zu is not a base (0..3)", fn, seq[i], i);
    return 0;
}

/* ------------------------------------------------------------------ */
/* per-read symbols                                                     */
/* ------------------------------------------------------------------ */
static float map_local_one(const char *fn, const_scrappie_matrix tr, const int *seq, size_t L, bool vit, size_t *first, size_t *last, int *path) {
    if (!tr || !seq) { set_err("%s: null argument", fn); return NAN; }
    if (!sh_crf_post_ok(tr)) { set_err("%s: not a transition matrix of 25 rows and at least one block", fn); return NAN; }
    if (tr->nc > (size_t)INT32_MAX / 2) { set_err("%s: %zu blocks is too many", fn, tr->nc); return NAN; }
    if (map_local_target_ok(fn, seq, L)) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    DBuf &dtr = e->d_map_post;
    const size_t nfl = (tr->nc - 1) * tr->stride + 25;           /* as far as the last column's 25th float */
    if (dtr.ensure(nfl * 4)) return NAN;
    if (hipMemcpyAsync(dtr.p, tr->data.f, nfl * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess) { set_err("%s: upload failed", fn); return NAN; }
    std::vector<MapLocalJob> jobs(1);
    jobs[0].trans = 0; jobs[0].lane = (int)tr->stride; jobs[0].nblock = tr->nc; jobs[0].seq = seq; jobs[0].L = L;
    if (map_local_run(e, jobs, dtr.as<float>(), vit, false, vit && (first || path), nullptr)) {
        free(jobs[0].path);
        const std::string keep = g_err;
        (void)hipGetLastError();
        set_err("%s", keep.c_str());
        return NAN;
    }
    if (first) *first = jobs[0].first;
    if (last) *last = jobs[0].last;
    if (path && jobs[0].path) memcpy(path, jobs[0].path, (tr->nc + 1) * 4);
    free(jobs[0].path);
    return jobs[0].score;
}

extern "C" float map_crf_to_reference_viterbi(const_scrappie_matrix trans, int const *seq, size_t seqlen, size_t *first, size_t *last, int *path) {
    return map_local_one("map_crf_to_reference_viterbi", trans, seq, seqlen, true, first, last, path);
}
extern "C" float map_crf_to_reference_forward(const_scrappie_matrix trans, int const *seq, size_t seqlen) {
    return map_local_one("map_crf_to_reference_forward", trans, seq, seqlen, false, nullptr, nullptr, nullptr);
}

/* ------------------------------------------------------------------ */
/* batched                                                              */
/* ------------------------------------------------------------------ */
/* what a launch group holds so far: MapLoad, and the sequences already counted */
struct MapLocalLoad { size_t sumT = 0, maxT = 0, extra = 0; std::set<std::pair<const int *, size_t>> seqs; };

static void map_local_blank(scrappie_hip_map_local_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].path); r[i] = scrappie_hip_map_local_result{NAN, 0, (size_t)-1, 0, nullptr}; }
}
extern "C" void scrappie_hip_free_map_local_results(scrappie_hip_map_local_result *r, size_t n) { free_paths(r, n); }

/* one launch group: reads idx[] of the call */
static int map_local_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const scrappie_hip_map_local_target *tg, const std::vector<size_t> &idx,
                           const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_local_result *out, LaunchCut<MapLocalLoad> &cut) {
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const raw_table *> win;
    for (size_t r : idx) win.push_back(&reads[r]);
    RunOut ro;
    std::vector<unsigned> bad;
    if (run_staged(e, m, win, p, STOP_POST, 5, &ro, bad, e->map_ms)) return -1;
    const LaunchGroup &lg = e->current().lg;
    std::vector<MapLocalJob> jobs;
    std::vector<size_t> who;
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0) continue;
        const size_t r = idx[(size_t)o];
        if (bad[i]) {
            cut.refuse(r, "the read holds values outside the supported range (is the signal trimmed and med/MAD-normalised?)");
            continue;
        }
        MapLocalJob j;
        j.trans = lg.tile_boff[i >> 4]; j.lane = (int)(i & 15); j.nblock = (size_t)lg.rT[i]; j.seq = tg[r].seq; j.L = tg[r].seqlen;
        jobs.push_back(j);
        who.push_back(r);
    }
    const int rc = map_local_run(e, jobs, ro.E, vit, true, vit && want_path, e->map_ms + 1);
    for (size_t k = 0; k < jobs.size(); k++) {
        if (rc) { free(jobs[k].path); continue; }
        out[who[k]] = scrappie_hip_map_local_result{jobs[k].score, jobs[k].nblock, jobs[k].first, jobs[k].last, jobs[k].path};
    }
    return rc;
}

extern "C" int scrappie_hip_map_local_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_local_target *targets,
                                            size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_local_result *out) {
    if (!e || (n && (!reads || !targets || !out))) return set_err("map_local_batch: null argument");
    std::lock_guard<std::mutex> call(e->call_mu);
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_map_local_result{NAN, 0, (size_t)-1, 0, nullptr};
    Model *m = get_model(e, model);
    if (!m) return -1;
    if (m->arch != 1) return set_err("map_local_batch: model '%s' is a transducer model; reads are mapped into a longer sequence with flip-flop (CRF) models only", m->name.c_str());
    scrappie_hip_params dp = scrappie_hip_default_params();
    if (!p) p = &dp;
    (void)hipSetDevice(e->device);
    for (double &x : e->map_ms) x = 0.0;
    const bool vit = viterbi != 0, wp = want_path != 0;
    const long stride = (long)e->map_crf_local_stride;
    /* every distinct sequence of the call is checked once */
    std::map<std::pair<const int *, size_t>, std::string> checked;
    /* launch groups as scrappie_hip_map_batch cuts them; a read adds its windows, scores and scratch rows, the second pass's traceback, and its sequence
     * where no read of the group has brought it */
    const size_t bpb = bytes_per_block(m, true);
    const size_t budget = e->max_launch_blocks ? e->max_launch_blocks * bpb : (size_t)(e->mem_frac * (double)e->total_mem);
    auto cost = [&](size_t sT, size_t mT, size_t ex) { return (sT / 16 + mT + 1) * bpb + ex; };
    LaunchCut<MapLocalLoad> cut{e, "map_local_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLocalLoad &) { return map_local_group(e, m, reads, targets, grp, p, vit, wp, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        const scrappie_hip_map_local_target &t = targets[i];
        const size_t T = map_blocks(m, map_read_nsample(m, reads[i]));
        if (T == 0) { cut.refuse(i, "read too short for the model (or empty)"); continue; }
        if (T > (size_t)INT32_MAX / 2) { cut.refuse(i, "too many blocks"); continue; }
        const auto key = std::make_pair(t.seq, t.seqlen);
        auto it = checked.find(key);
        if (it == checked.end()) it = checked.emplace(key, map_local_target_ok("map_local_batch", t.seq, t.seqlen) ? std::string(g_err) : std::string()).first;
        if (!it->second.empty()) { cut.refuse(i, it->second.c_str()); continue; }
        const size_t rb = map_local_read_bytes(t.seqlen, T, stride, vit && wp), sb = t.seqlen * 4 + 16;
        if (cost(T, T, rb + sb) > budget) { cut.refuse(i, "read and sequence too long for one launch group on this device"); continue; }
        MapLocalLoad &g = cut.load;
        const bool seen = g.seqs.count(key) != 0;
        const bool fits = cut.who.size() < e->max_launch_reads && cost(g.sumT + T, std::max(g.maxT, T), g.extra + rb + (seen ? 0 : sb)) <= budget;
        cut.add(i, fits);                                          /* (a flush clears the load: the sequence counts again) */
        MapLocalLoad &h = cut.load;
        h.sumT += T; h.maxT = std::max(h.maxT, T); h.extra += rb + (h.seqs.insert(key).second ? sb : 0);
    }
    return cut.finish([&] { map_local_blank(out, n); },
                      [](size_t i, const char *why) { set_err("map_local_batch: read %zu: %s", i, why); });
}
