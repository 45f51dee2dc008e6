/* sh_eng_squig_local.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * raw signals mapped INTO a longer reference squiggle (k_squig_local, sh_squig_local.h).  scrappie_hip_squiggle_match_local_batch cuts a
 * call into launches (LaunchCut under "squiggle_budget_kb"); every distinct reference of the call is checked and put through
 * sh_squiggle_tables once, and uploaded once per launch.  Two passes, as sh_eng_map_local.inc: every window of every read of a launch in
 * ONE k_squig_local launch (per home), scores and end states back, the host picks each read's best window (or sums them); with a path
 * wanted a second launch runs the traceback on that window alone -- it must repeat the first pass's bits or the read fails -- and
 * k_squig_local_walk returns path, first and last.  squiggle_match_local_* are a batch of one on the process-default engine.  The cut
 * of a reference into windows is host arithmetic in sh_host.c (scrappie_hip_squiggle_local_plan).  No network runs and no model is
 * needed. */

/* launches of each k_squig_local form in this process: index (vit ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_squig_local_forms[4];
extern "C" void scrappie_hip_squiggle_local_form_counts(uint64_t forms[4]) {
    for (int k = 0; k < 4; k++) if (forms) forms[k] = g_squig_local_forms[k].load(std::memory_order_relaxed);
}

typedef std::tuple<const float *, size_t, size_t> SqlKey;      /* a reference as the caller names it: params, npos, stride */
static SqlKey sql_key(const scrappie_hip_squiggle_target &t) { return SqlKey(t.params, t.npos, t.stride); }

/* one distinct reference of a call: why it cannot be mapped into (empty: it can), its tables */
struct SqlRef { std::string why; std::vector<float> tab; };

/* what a launch holds so far */
struct SqlLoad { size_t bytes = 0, nwin = 0; std::set<SqlKey> refs; };

/* the four planes of moves (8 ceil(ncell / 64) words per sample) and the END plane (a quarter as many), whole 16-byte pieces */
static long long sql_tb_words(size_t ncell, size_t nsample) { return ((long long)nsample * (long long)(10 * ((ncell + 63) / 64)) + 3) & ~3LL; }

static long long sql_cut(size_t L, size_t ns, long stride, MapLocalCut *c) {
    const long long nw = scrappie_hip_squiggle_local_plan(L, ns, stride, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!c || nw <= 0) return nw;
    const size_t n = (size_t)nw;
    c->first.resize(n); c->ncell.resize(n); c->own.resize(n); c->home.resize(n); c->scr.resize(n);
    long long fl = 0;
    return scrappie_hip_squiggle_local_plan(L, ns, stride, n, c->first.data(), c->ncell.data(), c->own.data(), c->home.data(), c->scr.data(), &fl);
}

/* device bytes one read adds to a launch, its reference's tables apart: its samples, the first pass's windows, scores, end states and scratch
 * rows; with a path the second pass's traceback and rows on its largest window, and the path */
static size_t sql_read_bytes(size_t L, size_t ns, long stride, bool path, size_t *nwin) {
    long long fl = 0;
    const long long nw = scrappie_hip_squiggle_local_plan(L, ns, stride, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &fl);
    if (nwin) *nwin = (size_t)nw;
    size_t b = ns * 4 + (size_t)nw * (sizeof(ShSquigLocalWin) + 12) + (size_t)fl * 4 + 64;
    if (path) {
        const size_t s = scrappie_hip_squiggle_local_stride(L, ns, stride);
        const size_t nc = std::min(s + 2 * (ns - 1) + 1, L);
        b += (size_t)sql_tb_words(nc, ns) * 4 + ns * 4 + sh_squig_local_scr_floats(nc) * 4 + sizeof(ShSquigLocalWin) + 64;
    }
    return b;
}

/* one read of a launch */
struct SqlJob {
    size_t r;                   /* which read of the call */
    long long sig, tab;         /* where its samples and its reference's tables lie on the device */
    size_t ns, L;
    const MapLocalCut *cut;
    float score = NAN; int2 end = make_int2(0, 0);
};

/* the record of window w of job j; tb: its traceback's word offset, -1: none; scr_floats and lds take what it needs of its home */
static ShSquigLocalWin sql_win(const SqlJob &j, size_t w, long long tb, long long &scr_floats, size_t &lds) {
    const MapLocalCut &c = *j.cut;
    ShSquigLocalWin r{};
    r.sig = j.sig; r.tab = j.tab; r.tb = tb; r.nsample = (int)j.ns; r.npos = (int)j.L;
    r.first = (int)c.first[w]; r.ncell = (int)c.ncell[w]; r.own = (int)c.own[w]; r.ok = 1;
    r.own0 = w ? 1 : 0;                                  /* behind the cell kept for back state p0 - 1; window 0 has none */
    if (c.home[w]) { r.scr = scr_floats; scr_floats += (long long)sh_squig_local_scr_floats(c.ncell[w]); }
    else { r.scr = -1; lds = std::max(lds, sh_squig_local_lds_bytes(c.ncell[w])); }
    return r;
}

/* one launch of the windows wins[] through k_squig_local, in device order (dp_order: those of the LDS home first; perm[k]: which of wins[] goes
 * k-th); scores and, Viterbi, end states into dp_sql.h ([n] float, then [n] int2), which also has room for what a walk over path_len entries returns */
static int sql_launch(scrappie_hip_engine *e, const std::vector<ShSquigLocalWin> &wins, std::vector<size_t> &perm, size_t lds, long long scr_floats,
                      long long tb_words, long long path_len, ShSquigLocalArgs a, bool vit) {
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_sql;
    const size_t n = wins.size(), n_lds = dp_order(wins, perm);
    std::vector<ShSquigLocalWin> rd;                      /* (one home only: wins[] is in device order already) */
    if (n_lds && n_lds < n) { rd.resize(n); for (size_t k = 0; k < n; k++) rd[k] = wins[perm[k]]; }
    if (d.ensure(n, sizeof(ShSquigLocalWin), (tb_words + 3) & ~3LL, scr_floats, path_len, n * 24 + (size_t)path_len * 4 + 16, sizeof(int2))) return -1;
    HIPCHK(hipMemcpyAsync(d.rd.p, rd.empty() ? wins.data() : rd.data(), n * sizeof(ShSquigLocalWin), hipMemcpyHostToDevice, s));
    a.rd = d.rd.as<ShSquigLocalWin>(); a.tb = d.tb.as<unsigned>(); a.scr = d.scr.as<float>(); a.score = d.score.as<float>(); a.final_state = d.final_state.as<int2>();
    if (lds > SH_SQ_LDS) return set_err("squiggle_match_local_batch: a window of %zu bytes of LDS", lds);
    if (pick_bool([&](auto v) {
            return dp_launch<k_squig_local<v(), true>, k_squig_local<v(), false>>(s, a, n_lds, n, SH_SQ_NTH, lds, sh_squig_local_scr_lds_bytes(), g_squig_local_forms + (v() ? 2 : 0));
        }, vit)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d.h.p, d.score.p, n * 4, hipMemcpyDeviceToHost, s));
    if (vit) HIPCHK(hipMemcpyAsync((char *)d.h.p + n * 4, d.final_state.p, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    return 0;
}

/* one launch over the reads who[] of the call */
static int sql_run(scrappie_hip_engine *e, const std::vector<size_t> &who, const raw_table *reads, const scrappie_hip_squiggle_target *tg,
                   const std::map<SqlKey, SqlRef> &refs, const scrappie_hip_squiggle_params *p, bool vit, bool want_path,
                   scrappie_hip_squiggle_local_result *out, LaunchCut<SqlLoad> &cut) {
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_sql;
    const long stride = (long)e->squig_local_stride;
    const auto t0 = std::chrono::steady_clock::now();
    /* the references of the launch, each once; the signals end to end */
    std::map<SqlKey, long long> at;
    long long tab_floats = 0, sig_floats = 0;
    std::map<std::pair<size_t, size_t>, MapLocalCut> cut_of;      /* (positions, samples): reads of one length share a reference's cut */
    std::vector<SqlJob> jobs;
    std::vector<size_t> job_off(who.size() + 1, 0);
    for (size_t k = 0; k < who.size(); k++) {
        const size_t r = who[k];
        const SqlKey key = sql_key(tg[r]);
        if (at.emplace(key, tab_floats).second) tab_floats += (long long)(5 * tg[r].npos + 4);
        SqlJob j;
        j.r = r; j.ns = reads[r].end - reads[r].start; j.L = tg[r].npos; j.sig = sig_floats; j.tab = at[key];
        sig_floats += (long long)j.ns;
        auto found = cut_of.find(std::make_pair(j.L, j.ns));
        if (found == cut_of.end()) {
            found = cut_of.emplace(std::make_pair(j.L, j.ns), MapLocalCut()).first;
            (void)sql_cut(j.L, j.ns, stride, &found->second);
        }
        j.cut = &found->second;
        if (j.cut->first.empty()) return set_err("squiggle_match_local_batch: nothing to cut (a reference of %zu positions, %zu samples)", j.L, j.ns);
        job_off[k + 1] = job_off[k] + j.cut->first.size();
        jobs.push_back(j);
    }
    const size_t nj = jobs.size(), nwin = job_off[nj];
    if (e->d_sql_sig.ensure((size_t)sig_floats * 4 + 16) || e->d_sql_tab.ensure((size_t)tab_floats * 4 + 16) || e->h_sql.ensure((size_t)sig_floats * 4 + 16)) return -1;
    float *hsig = e->h_sql.as<float>();
    for (const SqlJob &j : jobs) memcpy(hsig + j.sig, reads[j.r].raw + reads[j.r].start, j.ns * 4);
    HIPCHK(hipMemcpyAsync(e->d_sql_sig.p, hsig, (size_t)sig_floats * 4, hipMemcpyHostToDevice, s));
    for (const auto &kv : at) {
        const std::vector<float> &tab = refs.at(kv.first).tab;
        HIPCHK(hipMemcpyAsync((char *)e->d_sql_tab.p + (size_t)kv.second * 4, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    }
    HIPCHK(sh_stream_wait(s));
    ShSquigLocalArgs a{};
    a.sig = e->d_sql_sig.as<float>(); a.tab = e->d_sql_tab.as<float>();
    a.move_back_pen = logf(p->prob_back); a.half_pen = logf(0.5f);          /* sh_squiggle_tables' pens */
    a.local_pen = p->local_pen; a.skip_pen = p->skip_pen; a.minscore = p->minscore;
    /* the first pass: window w of job k is job_off[k] + w */
    std::vector<ShSquigLocalWin> wins;
    std::vector<size_t> perm;
    long long scr_floats = 0;
    size_t lds = sh_squig_local_scr_lds_bytes();
    wins.reserve(nwin);
    for (size_t k = 0; k < nj; k++)
        for (size_t w = 0; w < jobs[k].cut->first.size(); w++) wins.push_back(sql_win(jobs[k], w, -1, scr_floats, lds));
    const auto t1 = std::chrono::steady_clock::now();
    if (sql_launch(e, wins, perm, lds, scr_floats, 0, 0, a, vit)) return -1;
    const auto t2 = std::chrono::steady_clock::now();
    std::vector<float> wsc(nwin);
    std::vector<int2> wend(vit ? nwin : 0);
    {
        const float *hs = d.h.as<float>();
        const int2 *he = (const int2 *)(hs + nwin);
        for (size_t k = 0; k < nwin; k++) { wsc[perm[k]] = hs[k]; if (vit) wend[perm[k]] = he[k]; }
    }
    /* per read: the highest window, the lowest on a tie; forward: sh_lse over the windows in their order */
    std::vector<size_t> bestw(nj, 0);
    for (size_t k = 0; k < nj; k++) {
        const float *sc = wsc.data() + job_off[k];
        const size_t nw = job_off[k + 1] - job_off[k];
        SqlJob &j = jobs[k];
        scrappie_hip_squiggle_local_result &res = out[j.r];
        res.n = reads[j.r].n;
        if (vit) {
            size_t b = 0;
            for (size_t w = 1; w < nw; w++) if (sc[w] > sc[b]) b = w;
            bestw[k] = b;
            j.score = sc[b];
            j.end = wend[job_off[k] + b];
            res.last = (size_t)j.end.x + 1;                  /* position states only move right: the path ends in, or left the reference from, its highest position */
        } else {
            float acc = sc[0];
            for (size_t w = 1; w < nw; w++) acc = map_local_lse(acc, sc[w]);
            j.score = acc;
        }
        res.score = j.score;
    }
    if (vit && want_path) {
        /* the second pass: each read's best window alone, with its traceback; perm[k]: the job that goes k-th on the device */
        long long tb_words = 0, scr2 = 0, path_len = 0;
        size_t lds2 = sh_squig_local_scr_lds_bytes();
        wins.clear();
        for (size_t k = 0; k < nj; k++) {
            wins.push_back(sql_win(jobs[k], bestw[k], tb_words, scr2, lds2));
            tb_words += sql_tb_words(jobs[k].cut->ncell[bestw[k]], jobs[k].ns);
            path_len += (long long)jobs[k].ns;
        }
        if (sql_launch(e, wins, perm, lds2, scr2, tb_words, path_len, a, true)) return -1;
        std::vector<long long> poff(nj);
        std::vector<char> bad(nj, 0);
        long long pend = 0;
        for (size_t k = 0; k < nj; k++) { poff[k] = pend; pend += (long long)jobs[perm[k]].ns; }
        {
            const float *hs = d.h.as<float>();               /* the same window again: the same bits */
            const int2 *he = (const int2 *)(hs + nj);
            for (size_t k = 0; k < nj; k++) {
                const SqlJob &j = jobs[perm[k]];
                if (memcmp(&hs[k], &j.score, 4) || he[k].x != j.end.x || he[k].y != j.end.y) {
                    char msg[240];
                    snprintf(msg, sizeof msg, "the second pass of a window disagrees with the first (%.9g at %d/%d, not %.9g at %d/%d)", hs[k], he[k].x, he[k].y,
                             j.score, j.end.x, j.end.y);
                    cut.refuse(j.r, msg);
                    bad[k] = 1;
                    poff[k] = -1;                            /* (not walked) */
                }
            }
        }
        if (e->d_sql_lohi.ensure(nj * 8 + 16)) return -1;
        HIPCHK(hipMemcpyAsync(d.path_off.p, poff.data(), nj * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_squig_local_walk, dim3((unsigned)((nj + 63) / 64)), dim3(64), 0, s, (const ShSquigLocalWin *)d.rd.p, (int)nj,
                           (const unsigned *)d.tb.p, (const int2 *)d.final_state.p, (const long long *)d.path_off.p, d.paths.as<int>(),
                           e->d_sql_lohi.as<int2>());
        HIPCHK(hipGetLastError());
        int32_t *hf = (int32_t *)d.h.p, *hp = hf + 2 * nj;
        HIPCHK(hipMemcpyAsync(hf, e->d_sql_lohi.p, nj * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hp, d.paths.p, (size_t)path_len * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
        for (size_t k = 0; k < nj; k++) {
            const SqlJob &j = jobs[perm[k]];
            scrappie_hip_squiggle_local_result &res = out[j.r];
            const raw_table &rt = reads[j.r];
            if (bad[k]) { res = scrappie_hip_squiggle_local_result{NAN, (size_t)-1, 0, 0, nullptr}; continue; }
            res.first = (size_t)hf[2 * k];
            res.last = (size_t)hf[2 * k + 1];
            res.path = (int32_t *)malloc(std::max<size_t>(rt.n, 1) * 4);
            if (!res.path) return set_err("out of host memory");
            for (size_t i = 0; i < rt.n; i++) res.path[i] = -1;
            memcpy(res.path + rt.start, hp + poff[k], j.ns * 4);
        }
    }
    const auto t3 = std::chrono::steady_clock::now();
    e->squig_ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    e->squig_ms[1] += std::chrono::duration<double, std::milli>(t2 - t1).count();
    e->squig_ms[2] += std::chrono::duration<double, std::milli>(t3 - t2).count();
    return 0;
}

static void sql_blank(scrappie_hip_squiggle_local_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].path); r[i] = scrappie_hip_squiggle_local_result{NAN, (size_t)-1, 0, 0, nullptr}; }
}
extern "C" void scrappie_hip_free_squiggle_local_results(scrappie_hip_squiggle_local_result *r, size_t n) { free_paths(r, n); }

extern "C" int scrappie_hip_squiggle_match_local_batch(scrappie_hip_engine *e, const raw_table *reads, const scrappie_hip_squiggle_target *targets,
                                                       size_t n, const scrappie_hip_squiggle_params *p, int viterbi, int want_path,
                                                       scrappie_hip_squiggle_local_result *out) {
    static const char *const fn = "squiggle_match_local_batch";
    if (!e || (n && (!reads || !targets || !out))) return set_err("%s: null argument", fn);
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_squiggle_local_result{NAN, (size_t)-1, 0, 0, nullptr};
    const scrappie_hip_squiggle_params dp = scrappie_hip_default_squiggle_params();
    if (!p) p = &dp;
    if (squig_params_ok(fn, p)) return -1;
    (void)hipSetDevice(e->device);
    { std::lock_guard<std::mutex> lk(e->mu); for (double &x : e->squig_ms) x = 0.0; }
    const bool vit = viterbi != 0, path = vit && want_path != 0;
    const long stride = (long)e->squig_local_stride;
    const size_t budget = launch_budget(e, e->dbg_squig_budget);
    const size_t skip = strlen(fn) + 2;                       /* (the checks' texts begin with the function's name) */
    std::map<SqlKey, SqlRef> refs;                            /* every distinct reference of the call: checked once, its tables made once */
    LaunchCut<SqlLoad> cut{e, fn};
    cut.run = [&](const std::vector<size_t> &who, SqlLoad &) { return sql_run(e, who, reads, targets, refs, p, vit, path, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (squig_signal_ok(fn, reads[i])) { cut.refuse(i, g_err + skip); continue; }
        const scrappie_hip_squiggle_target &t = targets[i];
        const SqlKey key = sql_key(t);
        auto it = refs.find(key);
        if (it == refs.end()) {
            it = refs.emplace(key, SqlRef()).first;
            if (squig_cand_ok(fn, t)) it->second.why = g_err + skip;
            else {
                const auto t0 = std::chrono::steady_clock::now();
                float pens[2];
                it->second.tab.resize(5 * t.npos + 4);
                sh_squiggle_tables(t.params, t.npos, t.stride, p->rate, p->prob_back, it->second.tab.data(), pens);
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                std::lock_guard<std::mutex> lk(e->mu);
                e->squig_ms[0] += ms;
            }
        }
        if (!it->second.why.empty()) { cut.refuse(i, it->second.why.c_str()); continue; }
        const size_t ns = reads[i].end - reads[i].start, tb = (5 * t.npos + 4) * 4 + 16;
        size_t nw = 0;
        const size_t rb = sql_read_bytes(t.npos, ns, stride, path, &nw);
        if (nw == 0 || rb + tb > budget || nw > ((size_t)1 << 24)) {
            char msg[200];
            snprintf(msg, sizeof msg, "%zu samples into %zu positions need %zu bytes on the device in %zu windows, more than one launch may take (%zu)", ns, t.npos,
                     rb + tb, nw, budget);
            cut.refuse(i, msg);
            continue;
        }
        const bool fits = cut.load.bytes + rb + (cut.load.refs.count(key) ? 0 : tb) <= budget && cut.load.nwin + nw <= ((size_t)1 << 24);
        cut.add(i, fits);                                     /* (a flush clears the load: the reference counts again) */
        cut.load.bytes += rb + (cut.load.refs.insert(key).second ? tb : 0);
        cut.load.nwin += nw;
    }
    return cut.finish([&] { sql_blank(out, n); }, [&](size_t i, const char *why) { set_err("%s: read %zu: %s", fn, i, why); });
}

/* ------------------------------------------------------------------ */
/* per-read symbols                                                     */
/* ------------------------------------------------------------------ */
static float sql_one(const char *fn, const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen, float skip_pen,
                     float minscore, bool vit, int32_t *path_padded, size_t *first, size_t *last) {
    if (!signal.raw) { set_err("%s: no signal", fn); return NAN; }
    if (!params || !params->data.f) { set_err("%s: no squiggle", fn); return NAN; }
    scrappie_hip_squiggle_params p;
    p.rate = rate; p.prob_back = prob_back; p.local_pen = local_pen; p.skip_pen = skip_pen; p.minscore = minscore;
    scrappie_hip_squiggle_target t;
    t.params = params->data.f; t.npos = params->nc; t.stride = params->stride;
    if (squig_params_ok(fn, &p) || squig_read_ok(fn, signal, t)) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    scrappie_hip_squiggle_local_result res;
    if (scrappie_hip_squiggle_match_local_batch(e, &signal, &t, 1, &p, vit ? 1 : 0, (vit && (path_padded || first)) ? 1 : 0, &res)) return NAN;
    if (std::isnan(res.score)) { free(res.path); return NAN; }           /* refused (its size): the text is set */
    if (first) *first = res.first;
    if (last) *last = res.last;
    if (path_padded && res.path) memcpy(path_padded, res.path, signal.n * 4);
    free(res.path);
    return res.score;
}

extern "C" float squiggle_match_local_viterbi(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                              float skip_pen, float minscore, int32_t *path_padded, size_t *first, size_t *last) {
    return sql_one("squiggle_match_local_viterbi", signal, rate, params, prob_back, local_pen, skip_pen, minscore, true, path_padded, first, last);
}
extern "C" float squiggle_match_local_forward(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                              float skip_pen, float minscore) {
    return sql_one("squiggle_match_local_forward", signal, rate, params, prob_back, local_pen, skip_pen, minscore, false, nullptr, nullptr, nullptr);
}
