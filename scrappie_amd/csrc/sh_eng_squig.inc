/* sh_eng_squig.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * mapping of raw signals to predicted squiggles (sh_squig.h).  scrappie_hip_squiggle_match_batch cuts a call into launches
 * whose traceback and scratch fit a share of the free device memory (LaunchCut, sh_eng_cut.inc); a launch is tables on the host
 * (sh_host.c) -> uploads -> k_squig in its two homes -> k_squig_walk -> scores and paths back (dp_order / dp_launch / dp_collect,
 * there too).  What is here is the family's own: the plan of a launch and what a read costs, the checks a read passes, the staging of
 * signals and tables.  The reference's squiggle_match_viterbi / _forward are a batch of one on the process-default engine.  No
 * network runs and no model is needed.  A read may carry a band (sh_squig_band.h: low[] per sample and one width); banded reads of
 * a call are cut into launches of their own (SquigBandPlan, squig_band_run: k_squig_band in its two homes -> k_squig_band_walk),
 * whose cost is the band's traceback and scratch, and unbanded reads take the launches they always took. */

/* host side of one launch: the reads' records (who[] of the cutter says whose), their signals and tables laid end to end, traceback / scratch offsets */
struct SquigPlan {
    std::vector<ShSquigRead> rd;
    std::vector<long long> path_off;      /* per read, -1: no path */
    long long sig_floats = 0, tab_floats = 0, tb_words = 0, scr_floats = 0, path_len = 0;
    size_t lds = SH_SQ_LDS_HEAD * 4;
    size_t bytes = 0;                     /* device bytes the launch holds so far */
};

static size_t squig_lds_bytes(size_t npos) { return (SH_SQ_LDS_HEAD + 2 * (2 * npos + 1) + 5 * npos + 4) * 4; }
/* code words (8 ceil(npos / 64) per sample) + END's source (one int32 per sample), rounded to whole 16-byte pieces */
static long long squig_tb_words(size_t npos, size_t nsample) {
    return (long long)nsample * sh_squig_words((int)npos) + (long long)((nsample + 3) & ~(size_t)3);
}
static long long squig_scr_floats(size_t npos) { return (long long)((2 * (2 * npos + 1) + 3) & ~(size_t)3); }
/* device bytes one read adds to a launch (signal, tables, traceback, path, scratch) */
static size_t squig_read_bytes(size_t npos, size_t nsample, bool path) {
    size_t b = nsample * 4 + (5 * npos + 4) * 4 + sizeof(ShSquigRead) + 64;
    if (path) b += (size_t)squig_tb_words(npos, nsample) * 4 + nsample * 4;
    if (npos > SH_SQ_LDS_MAX_POS) b += (size_t)squig_scr_floats(npos) * 4;
    return b;
}

static void squig_plan_add(SquigPlan &pl, size_t nsample, size_t npos, bool path) {
    ShSquigRead r{};
    r.nsample = (int)nsample; r.npos = (int)npos; r.ok = 1;
    r.sig = pl.sig_floats; pl.sig_floats += (long long)nsample;
    r.tab = pl.tab_floats; pl.tab_floats += (long long)(5 * npos + 4);
    r.tb = -1;
    if (path) {
        r.tb = pl.tb_words; pl.tb_words += squig_tb_words(npos, nsample);
        pl.path_off.push_back(pl.path_len); pl.path_len += (long long)nsample;
    } else pl.path_off.push_back(-1);
    if (npos <= SH_SQ_LDS_MAX_POS) { r.scr = -1; pl.lds = std::max(pl.lds, squig_lds_bytes(npos)); }
    else { r.scr = pl.scr_floats; pl.scr_floats += squig_scr_floats(npos); }
    pl.rd.push_back(r);
    pl.bytes += squig_read_bytes(npos, nsample, path);
}

/* The scratch part of the plan squig_plan_add makes of reads of npos[i] positions and nsample[i] samples, in this order in one
 * launch (no traceback): off[i] = the float offset of read i's two score rows in the scratch allocation, -1 where they live in
 * LDS; returns the floats the launch allocates for them all.  Host arithmetic only: for the tests, which hold it against what
 * k_squig touches (2 (2 npos + 1) floats from off[i]). */
extern "C" long long scrappie_hip_squiggle_plan_scratch(const size_t *npos, const size_t *nsample, size_t n, long long *off) {
    SquigPlan pl;
    for (size_t i = 0; i < n; i++) {
        squig_plan_add(pl, nsample[i], npos[i], false);
        if (off) off[i] = pl.rd[i].scr;
    }
    return pl.scr_floats;
}

/* launches of each k_squig form in this process: index (vit ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_squig_forms[4];

/* one launch over the reads who[] of the call: out[who] gets its score and, where the plan holds a path, its padded path (malloc'd, signal.n long) */
static int squig_run(scrappie_hip_engine *e, const std::vector<size_t> &who, SquigPlan &pl, const raw_table *reads, const scrappie_hip_squiggle_target *tg,
                     const scrappie_hip_squiggle_params *p, bool vit, scrappie_hip_squiggle_result *out) {
    const size_t n = pl.rd.size();
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_sq;
    const bool walk = vit && pl.path_len > 0;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<size_t> perm;
    const size_t n_lds = dp_order(pl.rd, perm);
    const size_t up_floats = ((size_t)pl.sig_floats + (size_t)pl.tab_floats + 1) & ~(size_t)1;      /* (the records behind them are 8-byte aligned) */
    if (d.ensure(n, sizeof(ShSquigRead), pl.tb_words, pl.scr_floats, pl.path_len, up_floats * 4 + n * (sizeof(ShSquigRead) + 8)) ||
        e->d_sq_sig.ensure((size_t)pl.sig_floats * 4 + 16) || e->d_sq_tab.ensure((size_t)pl.tab_floats * 4 + 16)) return -1;
    /* staging (pinned): signals | tables | records | path offsets */
    float *hsig = d.h.as<float>(), *htab = hsig + pl.sig_floats;
    ShSquigRead *hrd = (ShSquigRead *)(hsig + up_floats);
    long long *hoff = (long long *)(hrd + n);
    float pens[2] = {0.0f, 0.0f};
    for (size_t k = 0; k < n; k++) {
        const size_t i = perm[k];
        const ShSquigRead &r = pl.rd[i];
        const raw_table &rt = reads[who[i]];
        const scrappie_hip_squiggle_target &t = tg[who[i]];
        memcpy(hsig + r.sig, rt.raw + rt.start, (size_t)r.nsample * 4);
        sh_squiggle_tables(t.params, t.npos, t.stride, p->rate, p->prob_back, htab + r.tab, pens);
        hrd[k] = r; hoff[k] = pl.path_off[i];
    }
    HIPCHK(hipMemcpyAsync(e->d_sq_sig.p, hsig, (size_t)pl.sig_floats * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_sq_tab.p, htab, (size_t)pl.tab_floats * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.rd.p, hrd, n * sizeof(ShSquigRead), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.path_off.p, hoff, n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(sh_stream_wait(s));
    ShSquigArgs a{};
    a.rd = d.rd.as<ShSquigRead>(); a.sig = e->d_sq_sig.as<float>(); a.tab = e->d_sq_tab.as<float>(); a.tb = d.tb.as<unsigned>(); a.scr = d.scr.as<float>();
    a.score = d.score.as<float>(); a.final_state = d.final_state.as<int>();
    a.move_back_pen = pens[0]; a.half_pen = pens[1];
    a.local_pen = p->local_pen; a.skip_pen = p->skip_pen; a.minscore = p->minscore;
    const auto t1 = std::chrono::steady_clock::now();
    if (pick_bool([&](auto v) { return dp_launch<k_squig<v(), true>, k_squig<v(), false>>(s, a, n_lds, n, SH_SQ_NTH, pl.lds, SH_SQ_LDS_HEAD * 4, g_squig_forms + (v() ? 2 : 0)); },
                  vit)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    const auto t2 = std::chrono::steady_clock::now();
    if (dp_collect<k_squig_walk, ShSquigRead>(s, d, perm, pl.path_off, pl.path_len, walk, [&](size_t i, float sc, const int32_t *path) {
            scrappie_hip_squiggle_result &res = out[who[i]];
            const raw_table &rt = reads[who[i]];
            res.score = sc;
            res.n = rt.n;
            if (!path) return 0;
            res.path = (int32_t *)malloc(std::max<size_t>(rt.n, 1) * 4);
            if (!res.path) return set_err("out of host memory");
            for (size_t j = 0; j < rt.n; j++) res.path[j] = -1;
            memcpy(res.path + rt.start, path, (size_t)pl.rd[i].nsample * 4);
            return 0;
        })) return -1;
    const auto t3 = std::chrono::steady_clock::now();
    e->squig_ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    e->squig_ms[1] += std::chrono::duration<double, std::milli>(t2 - t1).count();
    e->squig_ms[2] += std::chrono::duration<double, std::milli>(t3 - t2).count();
    return 0;
}

/* ------------------------------------------------------------------ */
/* banded reads (sh_squig_band.h)                                       */
/* ------------------------------------------------------------------ */
/* host side of one launch of banded reads: as SquigPlan; low[] lies behind the signals, one int32 per sample at the signal's offset */
struct SquigBandPlan {
    std::vector<ShSquigBandRead> rd;
    std::vector<long long> path_off;
    long long sig_floats = 0, tab_floats = 0, tb_words = 0, scr_floats = 0, path_len = 0;
    size_t lds = SH_SQ_LDS_HEAD * 4;
    size_t bytes = 0;
};

static size_t squig_band_lds_bytes(size_t width) { return (SH_SQ_LDS_HEAD + 2 * (2 * width + 1)) * 4; }
/* code words (8 ceil(width / 64) per sample) + END's source, rounded to whole 16-byte pieces */
static long long squig_band_tb_words(size_t width, size_t nsample) {
    return (long long)nsample * sh_squig_words((int)width) + (long long)((nsample + 3) & ~(size_t)3);
}
/* device bytes one banded read adds to a launch (signal and low[], tables, the band's traceback, path, the band's scratch rows) */
static size_t squig_band_read_bytes(size_t npos, size_t width, size_t nsample, bool path) {
    size_t b = nsample * 8 + (5 * npos + 4) * 4 + sizeof(ShSquigBandRead) + 64;
    if (path) b += (size_t)squig_band_tb_words(width, nsample) * 4 + nsample * 4;
    if (width > SH_SQB_LDS_MAX_W) b += (size_t)squig_scr_floats(width) * 4;
    return b;
}

/* width: already at most npos (a wider band holds no more positions) */
static void squig_band_plan_add(SquigBandPlan &pl, size_t nsample, size_t npos, size_t width, bool path) {
    ShSquigBandRead r{};
    r.nsample = (int)nsample; r.npos = (int)npos; r.width = (int)width; r.ok = 1;
    r.sig = pl.sig_floats; pl.sig_floats += (long long)nsample;
    r.tab = pl.tab_floats; pl.tab_floats += (long long)(5 * npos + 4);
    r.tb = -1;
    if (path) {
        r.tb = pl.tb_words; pl.tb_words += squig_band_tb_words(width, nsample);
        pl.path_off.push_back(pl.path_len); pl.path_len += (long long)nsample;
    } else pl.path_off.push_back(-1);
    if (width <= SH_SQB_LDS_MAX_W) { r.scr = -1; pl.lds = std::max(pl.lds, squig_band_lds_bytes(width)); }
    else { r.scr = pl.scr_floats; pl.scr_floats += squig_scr_floats(width); }
    pl.rd.push_back(r);
    pl.bytes += squig_band_read_bytes(npos, width, nsample, path);
}

/* The plan squig_band_plan_add makes of banded reads in this order in one launch: scr_off[i] the float offset of read i's two rows
 * (2 (2 width + 1) floats) in the scratch allocation, -1 where they live in LDS; tb_off[i] its first traceback word, -1 without
 * want_path; scr_off[n] / tb_off[n] the floats / words the launch allocates for them all (each array may be NULL).  width[i] above
 * npos[i] counts as npos[i].  Returns the device bytes the cutter charges for the launch.  Host arithmetic only, for the tests. */
extern "C" long long scrappie_hip_squiggle_band_plan(const size_t *npos, const size_t *width, const size_t *nsample, size_t n, int want_path,
                                                     long long *scr_off, long long *tb_off) {
    SquigBandPlan pl;
    for (size_t i = 0; i < n; i++) {
        squig_band_plan_add(pl, nsample[i], npos[i], std::min(width[i], npos[i]), want_path != 0);
        if (scr_off) scr_off[i] = pl.rd[i].scr;
        if (tb_off) tb_off[i] = pl.rd[i].tb;
    }
    if (scr_off) scr_off[n] = pl.scr_floats;
    if (tb_off) tb_off[n] = pl.tb_words;
    return (long long)pl.bytes;
}

/* scrappy's diagonal band for the squiggle DP: width = min(npos, 2 h + 1), low[t] = clamp(floor(t npos / nsample) - h, 0, npos - width) */
extern "C" size_t scrappie_hip_squiggle_diagonal_band(size_t nsample, size_t npos, size_t halfwidth, int32_t *low) {
    if (npos == 0) return 0;
    const int64_t NPOS = (int64_t)npos, h = (int64_t)std::min(halfwidth, npos), width = std::min<int64_t>(NPOS, 2 * h + 1);
    if (low)
        for (size_t t = 0; t < nsample; t++)
            low[t] = (int32_t)std::min<int64_t>(std::max<int64_t>((int64_t)t * NPOS / (int64_t)nsample - h, 0), NPOS - width);
    return (size_t)width;
}

extern "C" size_t scrappie_hip_squiggle_band_lds_max_width(void) { return SH_SQB_LDS_MAX_W; }

/* launches of each k_squig_band form in this process: index (vit ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_squig_band_forms[4];
extern "C" void scrappie_hip_squiggle_band_form_counts(uint64_t forms[4]) {
    for (int k = 0; k < 4; k++) if (forms) forms[k] = g_squig_band_forms[k].load(std::memory_order_relaxed);
}

/* the checks a band passes before it reaches a kernel (ns samples in the window, npos positions); 0 or -1 with the reason */
static int squig_band_ok(const char *fn, const scrappie_hip_squiggle_band &b, size_t ns, size_t npos) {
    if (!b.low) return set_err("%s: a band of width %zu without low[]", fn, b.width);
    if (b.width == 0) return set_err("%s: a band of width 0", fn);
    for (size_t t = 0; t < ns; t++) {
        if (b.low[t] < 0) return set_err("%s: the band's low[%zu] = %d is negative", fn, t, (int)b.low[t]);
        if ((size_t)b.low[t] >= npos) return set_err("%s: the band's low[%zu] = %d is past the squiggle's %zu positions", fn, t, (int)b.low[t], npos);
        if (t && b.low[t] < b.low[t - 1]) return set_err("%s: the band's low[] decreases at sample %zu (%d after %d)", fn, t, (int)b.low[t], (int)b.low[t - 1]);
    }
    return 0;
}

/* squig_run for the banded reads who[] of the call; a read whose band admits no path is refused through the cutter (NAN, no path) */
static int squig_band_run(scrappie_hip_engine *e, const std::vector<size_t> &who, SquigBandPlan &pl, const raw_table *reads,
                          const scrappie_hip_squiggle_target *tg, const scrappie_hip_squiggle_band *bands, const scrappie_hip_squiggle_params *p, bool vit,
                          scrappie_hip_squiggle_result *out, LaunchCut<SquigBandPlan> &cut) {
    const size_t n = pl.rd.size();
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_sq;
    const bool walk = vit && pl.path_len > 0;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<size_t> perm;
    const size_t n_lds = dp_order(pl.rd, perm);
    const size_t up_floats = (2 * (size_t)pl.sig_floats + (size_t)pl.tab_floats + 1) & ~(size_t)1;
    if (d.ensure(n, sizeof(ShSquigBandRead), pl.tb_words, pl.scr_floats, pl.path_len, up_floats * 4 + n * (sizeof(ShSquigBandRead) + 8)) ||
        e->d_sq_sig.ensure(2 * (size_t)pl.sig_floats * 4 + 16) || e->d_sq_tab.ensure((size_t)pl.tab_floats * 4 + 16)) return -1;
    /* staging (pinned): signals | low[] | tables | records | path offsets */
    float *hsig = d.h.as<float>(), *htab = hsig + 2 * pl.sig_floats;
    int32_t *hlow = (int32_t *)(hsig + pl.sig_floats);
    const int *dlow = e->d_sq_sig.as<int>() + pl.sig_floats;
    ShSquigBandRead *hrd = (ShSquigBandRead *)(hsig + up_floats);
    long long *hoff = (long long *)(hrd + n);
    float pens[2] = {0.0f, 0.0f};
    for (size_t k = 0; k < n; k++) {
        const size_t i = perm[k];
        const ShSquigBandRead &r = pl.rd[i];
        const raw_table &rt = reads[who[i]];
        const scrappie_hip_squiggle_target &t = tg[who[i]];
        memcpy(hsig + r.sig, rt.raw + rt.start, (size_t)r.nsample * 4);
        memcpy(hlow + r.sig, bands[who[i]].low, (size_t)r.nsample * 4);
        sh_squiggle_tables(t.params, t.npos, t.stride, p->rate, p->prob_back, htab + r.tab, pens);
        hrd[k] = r; hrd[k].low = dlow + r.sig; hoff[k] = pl.path_off[i];
    }
    HIPCHK(hipMemcpyAsync(e->d_sq_sig.p, hsig, 2 * (size_t)pl.sig_floats * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_sq_tab.p, htab, (size_t)pl.tab_floats * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.rd.p, hrd, n * sizeof(ShSquigBandRead), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.path_off.p, hoff, n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(sh_stream_wait(s));
    ShSquigBandArgs a{};
    a.rd = d.rd.as<ShSquigBandRead>(); a.sig = e->d_sq_sig.as<float>(); a.tab = e->d_sq_tab.as<float>(); a.tb = d.tb.as<unsigned>(); a.scr = d.scr.as<float>();
    a.score = d.score.as<float>(); a.final_state = d.final_state.as<int>();
    a.move_back_pen = pens[0]; a.half_pen = pens[1];
    a.local_pen = p->local_pen; a.skip_pen = p->skip_pen; a.minscore = p->minscore;
    const auto t1 = std::chrono::steady_clock::now();
    if (pick_bool([&](auto v) { return dp_launch<k_squig_band<v(), true>, k_squig_band<v(), false>>(s, a, n_lds, n, SH_SQ_NTH, pl.lds, SH_SQ_LDS_HEAD * 4, g_squig_band_forms + (v() ? 2 : 0)); },
                  vit)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    const auto t2 = std::chrono::steady_clock::now();
    if (dp_collect<k_squig_band_walk, ShSquigBandRead>(s, d, perm, pl.path_off, pl.path_len, walk, [&](size_t i, float sc, const int32_t *path) {
            scrappie_hip_squiggle_result &res = out[who[i]];
            const raw_table &rt = reads[who[i]];
            if (sc < -SH_MAP_BIG / 2) {
                char msg[160];
                snprintf(msg, sizeof msg, "%s: the band admits no path (%d samples, %d positions, width %d)", cut.fn, pl.rd[i].nsample, pl.rd[i].npos, pl.rd[i].width);
                cut.refuse(who[i], msg);
                return 0;
            }
            res.score = sc;
            res.n = rt.n;
            if (!path) return 0;
            res.path = (int32_t *)malloc(std::max<size_t>(rt.n, 1) * 4);
            if (!res.path) return set_err("out of host memory");
            for (size_t j = 0; j < rt.n; j++) res.path[j] = -1;
            memcpy(res.path + rt.start, path, (size_t)pl.rd[i].nsample * 4);
            return 0;
        })) return -1;
    const auto t3 = std::chrono::steady_clock::now();
    e->squig_ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    e->squig_ms[1] += std::chrono::duration<double, std::milli>(t2 - t1).count();
    e->squig_ms[2] += std::chrono::duration<double, std::milli>(t3 - t2).count();
    return 0;
}

/* the checks a read and its squiggle pass before they reach a kernel; 0 or -1 with the reason */
static int squig_read_ok(const char *fn, const raw_table &rt, const scrappie_hip_squiggle_target &t) {
    if (!rt.raw) return set_err("%s: no signal", fn);
    if (!t.params) return set_err("%s: no squiggle", fn);
    if (rt.start >= rt.end) return set_err("%s: an empty signal window [%zu, %zu)", fn, rt.start, rt.end);
    if (rt.end > rt.n) return set_err("%s: the signal window ends at %zu, past its %zu samples", fn, rt.end, rt.n);
    if (rt.end - rt.start > (size_t)INT32_MAX / 2) return set_err("%s: %zu samples is too many", fn, rt.end - rt.start);
    if (t.npos == 0) return set_err("%s: a squiggle of no positions", fn);
    if (t.npos > SH_SQ_MAX_POS) return set_err("%s: a squiggle of %zu positions is longer than the %d this build maps", fn, t.npos, SH_SQ_MAX_POS);
    if (t.stride < 3) return set_err("%s: a squiggle column holds %zu floats (3: mean, log sd, dwell logit)", fn, t.stride);
    return 0;
}
static int squig_params_ok(const char *fn, const scrappie_hip_squiggle_params *p) {
    if (!(p->rate > 0.0f)) return set_err("%s: rate %g is not positive", fn, (double)p->rate);
    if (!(p->prob_back >= 0.0f && p->prob_back <= 1.0f)) return set_err("%s: prob_back %g is outside [0, 1]", fn, (double)p->prob_back);
    return 0;
}

extern "C" scrappie_hip_squiggle_params scrappie_hip_default_squiggle_params(void) {
    scrappie_hip_squiggle_params p;
    p.rate = 1.0f; p.prob_back = 0.0f; p.local_pen = 2.0f; p.skip_pen = 5000.0f; p.minscore = 5.0f;       /* scrappy's map_signal_to_squiggle */
    return p;
}

extern "C" size_t scrappie_hip_squiggle_lds_max_pos(void) { return SH_SQ_LDS_MAX_POS; }

extern "C" void scrappie_hip_launch_form_counts(uint64_t map_forms[16], uint64_t squig_forms[4]) {
    for (int k = 0; k < 16; k++) if (map_forms) map_forms[k] = g_map_forms[k].load(std::memory_order_relaxed);
    for (int k = 0; k < 4; k++) if (squig_forms) squig_forms[k] = g_squig_forms[k].load(std::memory_order_relaxed);
}

extern "C" void scrappie_hip_squiggle_timing(scrappie_hip_engine *e, double out[3]) { timing3(e ? e->squig_ms : nullptr, out); }
extern "C" void scrappie_hip_free_squiggle_results(scrappie_hip_squiggle_result *r, size_t n) { free_paths(r, n); }

extern "C" int scrappie_hip_squiggle_match_banded_batch(scrappie_hip_engine *e, const raw_table *reads, const scrappie_hip_squiggle_target *targets,
                                                        const scrappie_hip_squiggle_band *bands, size_t n, const scrappie_hip_squiggle_params *p, int viterbi,
                                                        int want_path, scrappie_hip_squiggle_result *out) {
    if (!e || (n && (!reads || !targets || !out))) return set_err("squiggle_match_batch: null argument");
    for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].n = 0; out[i].path = nullptr; }
    const scrappie_hip_squiggle_params dp = scrappie_hip_default_squiggle_params();
    if (!p) p = &dp;
    if (squig_params_ok("squiggle_match_batch", p)) return -1;
    (void)hipSetDevice(e->device);
    { std::lock_guard<std::mutex> lk(e->mu); for (double &x : e->squig_ms) x = 0.0; }
    const bool vit = viterbi != 0, path = vit && want_path != 0;
    const size_t budget = launch_budget(e, e->dbg_squig_budget);
    LaunchCut<SquigPlan> cut{e, "squiggle_match_batch"};          /* (the plan of the launch being assembled is the cutter's load) */
    cut.run = [&](const std::vector<size_t> &who, SquigPlan &pl) { return squig_run(e, who, pl, reads, targets, p, vit, out); };
    LaunchCut<SquigBandPlan> bcut{e, "squiggle_match_batch"};     /* the banded reads: launches of their own, in input order among themselves */
    bcut.run = [&](const std::vector<size_t> &who, SquigBandPlan &pl) { return squig_band_run(e, who, pl, reads, targets, bands, p, vit, out, bcut); };
    for (size_t i = 0; i < n && !cut.failed && !bcut.failed; i++) {
        if (squig_read_ok("squiggle_match_batch", reads[i], targets[i])) { cut.refuse(i, g_err); continue; }
        const size_t ns = reads[i].end - reads[i].start, npos = targets[i].npos;
        const bool banded = bands && (bands[i].low || bands[i].width);
        if (banded && squig_band_ok("squiggle_match_batch", bands[i], ns, npos)) { bcut.refuse(i, g_err); continue; }
        const size_t width = banded ? std::min(bands[i].width, npos) : 0;
        const size_t rb = banded ? squig_band_read_bytes(npos, width, ns, path) : squig_read_bytes(npos, ns, path);
        if (rb > budget) {
            char msg[160];
            snprintf(msg, sizeof msg, "squiggle_match_batch: %zu samples against %zu positions need %zu bytes on the device, more than one launch may take (%zu)", ns, npos, rb, budget);
            cut.refuse(i, msg);
            continue;
        }
        if (banded) {
            bcut.add(i, bcut.load.bytes + rb <= budget && bcut.who.size() < 65535);
            squig_band_plan_add(bcut.load, ns, npos, width, path);
        } else {
            cut.add(i, cut.load.bytes + rb <= budget && cut.who.size() < 65535);
            squig_plan_add(cut.load, ns, npos, path);
        }
    }
    /* the last launch of either kind; after a failed launch nothing more is launched and the call is blanked */
    if (!bcut.failed) cut.flush();
    if (!cut.failed) bcut.flush();
    if (cut.failed || bcut.failed) {
        scrappie_hip_free_squiggle_results(out, n);
        for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].n = 0; }
        return -1;
    }
    const bool first_banded = bcut.bad < cut.bad;
    if (std::min(cut.bad, bcut.bad) != (size_t)-1)
        set_err("%s (read %zu of the call)", first_banded ? bcut.why.c_str() : cut.why.c_str(), first_banded ? bcut.bad : cut.bad);
    return 0;
}

extern "C" int scrappie_hip_squiggle_match_batch(scrappie_hip_engine *e, const raw_table *reads, const scrappie_hip_squiggle_target *targets,
                                                 size_t n, const scrappie_hip_squiggle_params *p, int viterbi, int want_path,
                                                 scrappie_hip_squiggle_result *out) {
    return scrappie_hip_squiggle_match_banded_batch(e, reads, targets, nullptr, n, p, viterbi, want_path, out);
}

/* ------------------------------------------------------------------ */
/* per-read reference surface (decode.c:1035, :1262)                    */
/* ------------------------------------------------------------------ */
static float squig_one(const char *fn, const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                       float skip_pen, float minscore, bool vit, int32_t *path_padded, const int32_t *low = nullptr, size_t width = 0) {
    if (!signal.raw) { set_err("%s: no signal", fn); return NAN; }                   /* RETURN_NULL_IF, decode.c:1038-1040 */
    if (!params || !params->data.f) { set_err("%s: no squiggle", fn); return NAN; }
    if (vit && !path_padded) { set_err("%s: no path to write to", fn); return NAN; }
    scrappie_hip_squiggle_params p;
    p.rate = rate; p.prob_back = prob_back; p.local_pen = local_pen; p.skip_pen = skip_pen; p.minscore = minscore;
    scrappie_hip_squiggle_target t;
    t.params = params->data.f; t.npos = params->nc; t.stride = params->stride;
    if (squig_params_ok(fn, &p) || squig_read_ok(fn, signal, t)) return NAN;          /* the reference's asserts, and npos == 0 */
    const scrappie_hip_squiggle_band band = {low, width};
    if ((low || width) && squig_band_ok(fn, band, signal.end - signal.start, t.npos)) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    scrappie_hip_squiggle_result res;
    if (scrappie_hip_squiggle_match_banded_batch(e, &signal, &t, &band, 1, &p, vit ? 1 : 0, vit ? 1 : 0, &res)) return NAN;
    if (std::isnan(res.score)) { free(res.path); return NAN; }           /* refused (its band; its size): the text is set */
    if (vit) {
        if (!res.path) return NAN;
        memcpy(path_padded, res.path, signal.n * 4);
        free(res.path);
    }
    return res.score;
}

extern "C" float squiggle_match_viterbi(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                        float skip_pen, float minscore, int32_t *path_padded) {
    return squig_one("squiggle_match_viterbi", signal, rate, params, prob_back, local_pen, skip_pen, minscore, true, path_padded);
}
extern "C" float squiggle_match_forward(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                        float skip_pen, float minscore) {
    return squig_one("squiggle_match_forward", signal, rate, params, prob_back, local_pen, skip_pen, minscore, false, nullptr);
}
/* the same inside a band (sh_squig_band.h): low[] one entry per sample of the window and a width; low NULL and width 0: unbanded */
extern "C" float squiggle_match_viterbi_banded(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                               float skip_pen, float minscore, const int32_t *low, size_t width, int32_t *path_padded) {
    return squig_one("squiggle_match_viterbi_banded", signal, rate, params, prob_back, local_pen, skip_pen, minscore, true, path_padded, low, width);
}
extern "C" float squiggle_match_forward_banded(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                               float skip_pen, float minscore, const int32_t *low, size_t width) {
    return squig_one("squiggle_match_forward_banded", signal, rate, params, prob_back, local_pen, skip_pen, minscore, false, nullptr, low, width);
}
