/* sh_eng_squig_local.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * raw signals mapped INTO a longer reference squiggle (k_squig_local, sh_squig_local.h).  scrappie_hip_squiggle_match_local_batch cuts a
 * call into launches (LaunchCut under "squiggle_budget_kb"); every distinct reference of the call is checked and put through
 * sh_squiggle_tables once, and uploaded once per launch.  The two passes -- every window of every read of a launch in ONE k_squig_local launch
 * (per home), each read's best window (or their sum), with a path wanted that window again with its traceback, which must repeat the first
 * pass's bits or the read fails, and k_squig_local_walk for path, first and last -- are win_run's (sh_eng_win.inc).  What is here is the family's
 * own: its form counters, its WinTraits (size formulas, planner, launch, walk), the uploads of a launch, the batch call with its cost model.
 * squiggle_match_local_* are a batch of one on the process-default engine.  The cut of a reference into windows is host arithmetic in sh_host.c
 * (scrappie_hip_squiggle_local_plan).  No network runs and no model is needed. */

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

template <> struct WinTraits<ShSquigLocalWin> {
    using Args = ShSquigLocalArgs;
    using WalkOut = int2;                                 /* first, last */
    static constexpr const char *name = "squiggle_match_local_batch";
    static constexpr size_t lds_cap = SH_SQ_LDS;
    static constexpr auto walk = k_squig_local_walk;
    static DpBufs &bufs(scrappie_hip_engine *e) { return e->dp_sql; }
    static DBuf &walk_out(scrappie_hip_engine *e) { return e->d_sql_lohi; }
    static size_t lds_bytes(size_t ncell, const Args &) { return sh_squig_local_lds_bytes(ncell); }
    static long long scr_floats(size_t ncell) { return (long long)sh_squig_local_scr_floats(ncell); }
    /* the four planes of moves (8 ceil(ncell / 64) words per sample) and the END plane (a quarter as many), whole 16-byte pieces */
    static long long tb_words(size_t ncell, size_t nsample) { return ((long long)nsample * (long long)(10 * ((ncell + 63) / 64)) + 3) & ~3LL; }
    static size_t path_len(size_t nsample) { return nsample; }
    static size_t last_of(int2 end) { return (size_t)end.x + 1; }      /* position states only move right: the path ends in, or left the reference from, its highest position */
    static void walked(int2 w, size_t &first, size_t &last) { first = (size_t)w.x; last = (size_t)w.y; }
    static auto plan(long stride, size_t L, size_t ns) {
        return [=](size_t cap, size_t *first, size_t *ncell, size_t *own, int *home, long long *scr, long long *fl) {
            return scrappie_hip_squiggle_local_plan(L, ns, stride, cap, first, ncell, own, home, scr, fl);
        };
    }
    static int launch(hipStream_t s, const Args &a, size_t n_lds, size_t n, size_t lds, bool vit, bool) {
        return pick_bool([&](auto v) {
                return dp_launch<k_squig_local<v(), true>, k_squig_local<v(), false>>(s, a, n_lds, n, SH_SQ_NTH, lds, sh_squig_local_scr_lds_bytes(), g_squig_local_forms + (v() ? 2 : 0));
            }, vit);
    }
};

/* device bytes one read adds to a launch, its reference's tables apart: its samples and what win_read_bytes counts */
static size_t sql_read_bytes(size_t L, size_t ns, long stride, bool path, size_t *nwin) {
    const size_t nc2 = std::min(scrappie_hip_squiggle_local_stride(L, ns, stride) + 2 * (ns - 1) + 1, L);
    return ns * 4 + win_read_bytes<ShSquigLocalWin>(WinTraits<ShSquigLocalWin>::plan(stride, L, ns), ns, nc2, path, nwin);
}

/* one launch over the reads who[] of the call: the references' tables and the signals up (squig_ms[0]), then both passes (win_run: squig_ms[1] from the
 * building of the window records through the first pass, squig_ms[2] the rest).  A read whose second pass disagrees with its first is refused alone. */
static int sql_run(scrappie_hip_engine *e, const std::vector<size_t> &who, const raw_table *reads, const scrappie_hip_squiggle_target *tg,
                   const std::map<SqlKey, SqlRef> &refs, const scrappie_hip_squiggle_params *p, bool vit, bool want_path,
                   scrappie_hip_squiggle_local_result *out, LaunchCut<SqlLoad> &cut) {
    using T = WinTraits<ShSquigLocalWin>;
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    const long stride = (long)e->squig_local_stride;
    const auto t0 = std::chrono::steady_clock::now();
    /* the references of the launch, each once; the signals end to end */
    std::map<SqlKey, long long> at;
    long long tab_floats = 0, sig_floats = 0;
    WinCuts cuts;
    std::vector<WinJob> jobs;
    std::vector<long long> sig_at, tab_at;      /* where a job's samples and its reference's tables lie on the device */
    for (const size_t r : who) {
        const SqlKey key = sql_key(tg[r]);
        if (at.emplace(key, tab_floats).second) tab_floats += (long long)(5 * tg[r].npos + 4);
        const size_t ns = reads[r].end - reads[r].start, L = tg[r].npos;
        jobs.push_back(WinJob{ns, L, cuts.get(L, ns, T::plan(stride, L, ns))});
        sig_at.push_back(sig_floats); tab_at.push_back(at[key]);
        sig_floats += (long long)ns;
    }
    if (e->d_sql_sig.ensure((size_t)sig_floats * 4 + 16) || e->d_sql_tab.ensure((size_t)tab_floats * 4 + 16) || e->h_sql.ensure((size_t)sig_floats * 4 + 16)) return -1;
    float *hsig = e->h_sql.as<float>();
    for (size_t k = 0; k < who.size(); k++) memcpy(hsig + sig_at[k], reads[who[k]].raw + reads[who[k]].start, jobs[k].rows * 4);
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
    e->squig_ms[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return win_run<ShSquigLocalWin>(e, jobs, a, vit, false, want_path, e->squig_ms + 1, Span2(),
        [&](size_t k, size_t w) {
            ShSquigLocalWin r{};
            r.sig = sig_at[k]; r.tab = tab_at[k]; r.nsample = (int)jobs[k].rows; r.npos = (int)jobs[k].L;
            r.own0 = w ? 1 : 0;                              /* behind the cell kept for back state p0 - 1; window 0 has none */
            return r;
        },
        [&](size_t k, const char *why) { cut.refuse(who[k], why); return 0; },
        [&](size_t k, float score, int2, size_t first, size_t last, const int32_t *path) {
            const raw_table &rt = reads[who[k]];
            scrappie_hip_squiggle_local_result &res = out[who[k]];
            res.score = score; res.n = rt.n; res.first = first; res.last = last;
            if (!path) return 0;
            res.path = (int32_t *)malloc(std::max<size_t>(rt.n, 1) * 4);
            if (!res.path) return set_err("out of host memory");
            for (size_t i = 0; i < rt.n; i++) res.path[i] = -1;
            memcpy(res.path + rt.start, path, jobs[k].rows * 4);
            return 0;
        });
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
