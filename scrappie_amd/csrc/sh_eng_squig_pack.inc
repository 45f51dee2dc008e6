/* sh_eng_squig_pack.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * one raw signal against many candidate squiggles (k_squig_pack, sh_squig_pack.h).  scrappie_hip_squiggle_match_multi_batch cuts a call into
 * launches (LaunchCut); a launch is: every read's signal staged and uploaded ONCE, the tables and cell words of every distinct cand array of the
 * launch uploaded once (PackLaunch, sh_eng_post.inc), every pack of every read a workgroup of one k_squig_pack launch, the candidates too long for
 * a pack through k_squig on the same call (squig_run, sh_eng_squig.inc), scores back; with a path wanted, a second pass of squig_run on each
 * read's best candidate alone, so the path is scrappie_hip_squiggle_match_batch's by construction.  The packing itself is host arithmetic in
 * sh_host.c (scrappie_hip_squiggle_pack_plan, sh_squig_pack_layout).  No network runs, so nothing of PostCall / post_group applies; the sets of a
 * call are PackSets' (sh_eng_post.inc). */

#define SH_SQUIG_PACK_CELLS 512       /* cells a pack holds unless the debug option "squig_pack_cells" says otherwise: the fastest on 24 barcodes of 40 positions, 12.4 % ahead of 256 (profiles/squiggle_pack_rate.txt) */

/* launches of each k_squig_pack form in this process: index viterbi */
static std::atomic<uint64_t> g_squig_pack_forms[2];
extern "C" void scrappie_hip_squiggle_pack_form_counts(uint64_t forms[2]) {
    for (int k = 0; k < 2; k++) if (forms) forms[k] = g_squig_pack_forms[k].load(std::memory_order_relaxed);
}

/* a PackSet (sh_eng_post.inc) of candidate squiggles: checked, through sh_squiggle_tables and packed as k_squig_pack reads it, once; cellw holds per
 * pack 7 ncell + 7 ncand words (sh_internal.h), floats as their bits; firsts stays empty; bytes: the read's samples apart */
struct SquigCandSet : PackSetOf<scrappie_hip_squiggle_target> {
    std::vector<int> npiece;                  /* per pack */
    std::vector<size_t> over;                 /* the candidates that take k_squig */
    size_t maxpos = 0;                        /* the longest candidate that can be matched */
    size_t lds = 0;                           /* dynamic LDS of its largest pack */
};

static int squig_cand_ok(const char *fn, const scrappie_hip_squiggle_target &t) {
    if (!t.params) return set_err("%s: no squiggle", fn);
    if (t.npos == 0) return set_err("%s: a squiggle of no positions", fn);
    if (t.npos > SH_SQ_MAX_POS) return set_err("%s: a squiggle of %zu positions is longer than the %d this build maps", fn, t.npos, SH_SQ_MAX_POS);
    if (t.stride < 3) return set_err("%s: a squiggle column holds %zu floats (3: mean, log sd, dwell logit)", fn, t.stride);
    return 0;
}
static int squig_signal_ok(const char *fn, const raw_table &rt) {
    if (!rt.raw) return set_err("%s: no signal", fn);
    if (rt.start >= rt.end) return set_err("%s: an empty signal window [%zu, %zu)", fn, rt.start, rt.end);
    if (rt.end > rt.n) return set_err("%s: the signal window ends at %zu, past its %zu samples", fn, rt.end, rt.n);
    if (rt.end - rt.start > (size_t)INT32_MAX / 2) return set_err("%s: %zu samples is too many", fn, rt.end - rt.start);
    return 0;
}

/* pack_cells 0: every candidate through k_squig.  A candidate that the plan leaves alone in its pack shares the pack's barrier with nobody and is
 * 1.8 times slower there than in k_squig (profiles/squiggle_pack_rate.txt), so it takes k_squig too unless lone says otherwise. */
static void squig_cand_set_build(SquigCandSet &cs, const char *fn, const scrappie_hip_squiggle_target *cand, size_t n, const scrappie_hip_squiggle_params *p,
                                 size_t pack_cells, bool lone) {
    cs.cand = cand; cs.n = n;
    std::vector<size_t> good, len;
    const std::string pre = std::string(fn) + ": ";
    for (size_t k = 0; k < n; k++) {
        if (squig_cand_ok(fn, cand[k])) {
            if (cs.why.empty()) cs.why = "candidate " + std::to_string(k) + ": " + (strncmp(g_err, pre.c_str(), pre.size()) ? g_err : g_err + pre.size());
            continue;
        }
        good.push_back(k); len.push_back(cand[k].npos);
        cs.maxpos = std::max(cs.maxpos, cand[k].npos);
    }
    std::vector<int> pack(good.size(), -1);
    std::vector<long long> cell(good.size(), -1);
    size_t npack = (pack_cells && !good.empty()) ? (size_t)scrappie_hip_squiggle_pack_plan(len.data(), good.size(), pack_cells, pack.data(), cell.data()) : 0;
    if (!lone && npack) {          /* the packs of one candidate dissolved, the others renumbered in their order */
        std::vector<int> members(npack, 0), renum(npack, -1);
        for (int q : pack) if (q >= 0) members[(size_t)q]++;
        size_t kept = 0;
        for (size_t q = 0; q < npack; q++) if (members[q] > 1) renum[q] = (int)kept++;
        for (int &q : pack) if (q >= 0) q = renum[(size_t)q];
        npack = kept;
    }
    std::vector<std::vector<size_t>> mem(npack), mlen(npack);
    for (size_t i = 0; i < good.size(); i++)
        if (pack[i] >= 0) { mem[(size_t)pack[i]].push_back(good[i]); mlen[(size_t)pack[i]].push_back(len[i]); }
    std::vector<float> tab;
    float pens[2];
    auto putf = [](int *dst, float v) { memcpy(dst, &v, 4); };          /* (the words are uploaded as one array; the kernel reads these as floats) */
    for (size_t q = 0; q < npack; q++) {
        const size_t NK = mem[q].size(), NC = std::accumulate(mlen[q].begin(), mlen[q].end(), (size_t)0), w0 = cs.cellw.size();
        cs.cellw.resize(w0 + SH_SQP_IN_CELL_WORDS * NC + SH_SQP_IN_CAND_WORDS * NK);
        int *const loc = cs.cellw.data() + w0, *const scale = loc + NC, *const logsc = scale + NC, *const move = logsc + NC, *const stay = move + NC;
        int *const wa = stay + NC, *const wb = wa + NC, *const first = wb + NC, *const npos = first + NK, *const piece0 = npos + NK, *const npiece = piece0 + NK;
        int *const move0 = npiece + NK, *const stay0 = move0 + NK, *const stayE = stay0 + NK;
        const size_t NP = sh_squig_pack_layout(mlen[q].data(), NK, wa, wb, piece0, npiece);
        size_t f = 0;
        for (size_t m = 0; m < NK; m++) {
            const scrappie_hip_squiggle_target &t = cand[mem[q][m]];
            const size_t L = t.npos;
            tab.resize(5 * L + 4);
            sh_squiggle_tables(t.params, L, t.stride, p->rate, p->prob_back, tab.data(), pens);
            const float *mp = tab.data() + 3 * L, *sp = tab.data() + 4 * L + 2;
            for (size_t i = 0; i < L; i++) {
                putf(loc + f + i, tab[i]); putf(scale + f + i, tab[L + i]); putf(logsc + f + i, tab[2 * L + i]);
                putf(move + f + i, mp[i + 1]); putf(stay + f + i, sp[i + 1]);
            }
            first[m] = (int)f; npos[m] = (int)L;
            putf(move0 + m, mp[0]); putf(stay0 + m, sp[0]); putf(stayE + m, sp[L + 1]);
            f += L;
        }
        cs.packs.push_back(PackSet::Pack{w0, 0, cs.packed.size(), NC, NK});
        cs.npiece.push_back((int)NP);
        cs.lds = std::max(cs.lds, sh_squig_pack_lds_bytes(NC, NK, NP));
        cs.packed.insert(cs.packed.end(), mem[q].begin(), mem[q].end());
    }
    for (size_t i = 0; i < good.size(); i++)
        if (pack[i] < 0) {
            cs.over.push_back(good[i]);
            cs.bytes += squig_read_bytes(len[i], 0, false);
        }
    cs.bytes += (cs.cellw.size() + n) * 4 + cs.packs.size() * sizeof(ShSquigPack) + 64;
}

static size_t squig_pack_cells(const scrappie_hip_engine *e) { return e->squig_pack_cells < 0 ? (size_t)SH_SQUIG_PACK_CELLS : (size_t)e->squig_pack_cells; }

/* what a launch holds so far */
struct SquigMultiLoad { size_t bytes = 0, nover = 0; };

/* one read of a launch: which read of the call, its candidates, and where their scores go ([cs->n], NAN already) */
struct SquigMultiJob { size_t r; const SquigCandSet *cs; float *score; };

/* pairs (read, candidate) through squig_run as a batch of their own: scores into score[], with path the padded paths into paths[] (malloc'd) */
static int squig_multi_pairs(scrappie_hip_engine *e, const std::vector<raw_table> &rd, const std::vector<scrappie_hip_squiggle_target> &tg,
                             const scrappie_hip_squiggle_params *p, bool vit, bool path, float *score, int32_t **paths) {
    const size_t n = rd.size();
    if (n == 0) return 0;
    SquigPlan pl;
    std::vector<size_t> who(n);
    std::iota(who.begin(), who.end(), (size_t)0);
    for (size_t i = 0; i < n; i++) squig_plan_add(pl, rd[i].end - rd[i].start, tg[i].npos, path);
    std::vector<scrappie_hip_squiggle_result> res(n, scrappie_hip_squiggle_result{NAN, 0, nullptr});
    if (squig_run(e, who, pl, rd.data(), tg.data(), p, vit, res.data())) {
        free_paths(res.data(), n);
        return -1;
    }
    for (size_t i = 0; i < n; i++) {
        score[i] = res[i].score;
        if (paths) paths[i] = res[i].path; else free(res[i].path);
    }
    return 0;
}

/* one launch over the reads who[] of the call */
static int squig_multi_run(scrappie_hip_engine *e, const std::vector<size_t> &who, const raw_table *reads, const std::vector<const SquigCandSet *> &setof,
                           const scrappie_hip_squiggle_params *p, bool vit, bool want_path, scrappie_hip_squiggle_multi_result *out) {
    std::vector<SquigMultiJob> jobs;
    for (size_t r : who) jobs.push_back(SquigMultiJob{r, setof[r], out[r].score});
    {       /* the packs: one k_squig_pack launch, under the engine's lock */
        std::lock_guard<std::mutex> lk(e->mu);
        hipStream_t s = e->stream;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<long long> sig0(jobs.size(), 0);
        size_t nsig = 0;
        for (size_t j = 0; j < jobs.size(); j++) {
            if (jobs[j].cs->packs.empty()) continue;
            sig0[j] = (long long)nsig;
            nsig += reads[jobs[j].r].end - reads[jobs[j].r].start;
        }
        std::vector<ShSquigPack> pk;
        PackLaunch<SquigCandSet> L;
        L.lay(jobs, [&](size_t j, const PackSet::Pack &P, size_t cell, size_t, size_t o) {
            const raw_table &rt = reads[jobs[j].r];
            ShSquigPack q{};
            q.sig = sig0[j]; q.cell = (long long)cell; q.out = (long long)o;
            q.nsample = (int)(rt.end - rt.start); q.ncell = (int)P.ncell; q.ncand = (int)P.nitem;
            q.npiece = jobs[j].cs->npiece[(size_t)(&P - jobs[j].cs->packs.data())];
            pk.push_back(q);
        });
        if (!pk.empty()) {
            size_t lds = 0;
            for (const auto &kv : L.up) lds = std::max(lds, kv.first->lds);
            if (lds > SH_SQ_LDS) return set_err("squiggle_match_multi_batch: a pack of %zu bytes of LDS", lds);
            const size_t nscore = L.nscore;
            if (e->d_sqp_rd.ensure(pk.size() * sizeof(ShSquigPack)) || e->d_sqp_sig.ensure(nsig * 4 + 16) || e->d_sqp_w.ensure(L.cellw.size() * 4 + 16) ||
                e->d_sqp_score.ensure(nscore * 4 + 16) || e->h_sqp.ensure(std::max(nsig, nscore) * 4 + 16)) return -1;
            float *hsig = e->h_sqp.as<float>();
            for (size_t j = 0; j < jobs.size(); j++) {
                if (jobs[j].cs->packs.empty()) continue;
                const raw_table &rt = reads[jobs[j].r];
                memcpy(hsig + sig0[j], rt.raw + rt.start, (rt.end - rt.start) * 4);
            }
            HIPCHK(hipMemcpyAsync(e->d_sqp_sig.p, hsig, nsig * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(e->d_sqp_w.p, L.cellw.data(), L.cellw.size() * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(e->d_sqp_rd.p, pk.data(), pk.size() * sizeof(ShSquigPack), hipMemcpyHostToDevice, s));
            HIPCHK(sh_stream_wait(s));
            ShSquigPackArgs a{};
            a.pk = e->d_sqp_rd.as<ShSquigPack>(); a.sig = e->d_sqp_sig.as<float>(); a.words = e->d_sqp_w.as<int>(); a.score = e->d_sqp_score.as<float>();
            a.move_back_pen = logf(p->prob_back); a.half_pen = logf(0.5f);          /* sh_squiggle_tables' pens */
            a.local_pen = p->local_pen; a.skip_pen = p->skip_pen; a.minscore = p->minscore;
            const auto t1 = std::chrono::steady_clock::now();
            g_squig_pack_forms[vit ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
            if (pick_bool([&](auto v) { return launch_k<k_squig_pack<v()>>(dim3((unsigned)pk.size()), dim3(SH_SQ_NTH), lds, s, a); }, vit)) return -1;
            HIPCHK(hipGetLastError());
            HIPCHK(sh_stream_wait(s));
            const auto t2 = std::chrono::steady_clock::now();
            const float *hs = e->h_sqp.as<float>();
            HIPCHK(hipMemcpyAsync(e->h_sqp.p, e->d_sqp_score.p, nscore * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(sh_stream_wait(s));
            L.scatter(jobs, [&](const SquigMultiJob &job, size_t k, size_t slot) { job.score[k] = hs[slot]; });
            const auto t3 = std::chrono::steady_clock::now();
            e->squig_ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
            e->squig_ms[1] += std::chrono::duration<double, std::milli>(t2 - t1).count();
            e->squig_ms[2] += std::chrono::duration<double, std::milli>(t3 - t2).count();
        }
    }
    /* the candidates left to k_squig, then each read's best candidate alone with its traceback (squig_run takes the lock itself) */
    std::vector<raw_table> rd;
    std::vector<scrappie_hip_squiggle_target> tg;
    std::vector<std::pair<size_t, size_t>> pair;          /* (job, candidate) */
    for (size_t j = 0; j < jobs.size(); j++)
        for (size_t k : jobs[j].cs->over) { rd.push_back(reads[jobs[j].r]); tg.push_back(jobs[j].cs->cand[k]); pair.emplace_back(j, k); }
    if (!pair.empty()) {
        std::vector<float> sc(pair.size(), NAN);
        if (squig_multi_pairs(e, rd, tg, p, vit, false, sc.data(), nullptr)) return -1;
        for (size_t i = 0; i < pair.size(); i++) jobs[pair[i].first].score[pair[i].second] = sc[i];
    }
    rd.clear(); tg.clear();
    std::vector<size_t> second;
    for (const SquigMultiJob &job : jobs) {
        scrappie_hip_squiggle_multi_result &res = out[job.r];
        res.n = reads[job.r].n;
        res.best = best_finite(res.score, res.ncand);
        if (!(vit && want_path) || res.best < 0) continue;
        rd.push_back(reads[job.r]); tg.push_back(job.cs->cand[res.best]); second.push_back(job.r);
    }
    if (!second.empty()) {
        std::vector<float> sc(second.size(), NAN);
        std::vector<int32_t *> paths(second.size(), nullptr);
        if (squig_multi_pairs(e, rd, tg, p, true, true, sc.data(), paths.data())) return -1;
        for (size_t i = 0; i < second.size(); i++) out[second[i]].path = paths[i];
    }
    return 0;
}

static void squig_multi_blank(scrappie_hip_squiggle_multi_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].score); free(r[i].path); r[i] = scrappie_hip_squiggle_multi_result{nullptr, 0, -1, 0, nullptr}; }
}
extern "C" void scrappie_hip_free_squiggle_multi_results(scrappie_hip_squiggle_multi_result *r, size_t n) { if (r) squig_multi_blank(r, n); }

extern "C" int scrappie_hip_squiggle_match_multi_batch(scrappie_hip_engine *e, const raw_table *reads, const scrappie_hip_squiggle_candidates *cands,
                                                       size_t n, const scrappie_hip_squiggle_params *p, int viterbi, int want_path,
                                                       scrappie_hip_squiggle_multi_result *out) {
    static const char *const fn = "squiggle_match_multi_batch";
    if (!e || (n && (!reads || !cands || !out))) return set_err("%s: null argument", fn);
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_squiggle_multi_result{nullptr, 0, -1, 0, nullptr};
    const scrappie_hip_squiggle_params dp = scrappie_hip_default_squiggle_params();
    if (!p) p = &dp;
    if (squig_params_ok(fn, p)) return -1;
    (void)hipSetDevice(e->device);
    { std::lock_guard<std::mutex> lk(e->mu); for (double &x : e->squig_ms) x = 0.0; }
    const bool vit = viterbi != 0, path = vit && want_path != 0;
    /* the candidates: one set per distinct cand array of the call */
    PackSets<SquigCandSet> sets;
    std::vector<const SquigCandSet *> &setof = sets.of;
    setof.assign(n, nullptr);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = cands[i].ncand;
        out[i].score = (float *)malloc(std::max<size_t>(nc, 1) * sizeof(float));
        if (!out[i].score) { squig_multi_blank(out, n); return set_err("%s: out of host memory", fn); }
        std::fill(out[i].score, out[i].score + nc, NAN);
        out[i].ncand = nc;
        if (!nc || !cands[i].cand) continue;
        setof[i] = sets.get(cands[i].cand, nc, [&](SquigCandSet &cs) { squig_cand_set_build(cs, fn, cands[i].cand, nc, p, squig_pack_cells(e), e->squig_pack_lone); });
    }
    /* a read is charged for its signal (once for the packs, once per candidate left to k_squig), its set's tables, pack records and scores, the
     * scratch rows of the candidates left to k_squig and, with a path, the second pass on its longest candidate */
    const size_t budget = launch_budget(e, e->dbg_squig_budget);
    LaunchCut<SquigMultiLoad> cut{e, fn};
    cut.run = [&](const std::vector<size_t> &who, SquigMultiLoad &) { return squig_multi_run(e, who, reads, setof, p, vit, path, out); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (cands[i].ncand && !cands[i].cand) { cut.refuse(i, "no candidates"); continue; }
        if (squig_signal_ok(fn, reads[i])) { cut.refuse(i, g_err + strlen(fn) + 2); continue; }
        out[i].n = reads[i].n;
        const SquigCandSet *cs = setof[i];
        if (!cs) continue;                                             /* no candidates: a read with no scores */
        if (!cs->why.empty()) cut.refuse(i, cs->why.c_str());          /* (its other candidates are scored) */
        if (cs->packed.empty() && cs->over.empty()) continue;
        const size_t ns = reads[i].end - reads[i].start;
        const size_t rb = ns * 4 * (1 + cs->over.size()) + 64 + cs->bytes + (path ? squig_read_bytes(cs->maxpos, ns, true) : 0);
        if (rb > budget || cs->over.size() >= 65535) {
            char msg[200];
            snprintf(msg, sizeof msg, "%zu samples against %zu candidates need %zu bytes on the device, more than one launch may take (%zu)", ns, cs->n, rb, budget);
            cut.refuse(i, msg);
            continue;
        }
        cut.add(i, cut.load.bytes + rb <= budget && cut.who.size() < 65535 && cut.load.nover + cs->over.size() < 65535);
        cut.load.bytes += rb; cut.load.nover += cs->over.size();
    }
    return cut.finish([&] { squig_multi_blank(out, n); }, [&](size_t i, const char *why) { set_err("%s: read %zu: %s", fn, i, why); });
}

extern "C" int scrappie_hip_squiggle_match_multi(const raw_table signal, const scrappie_hip_squiggle_target *cand, size_t ncand,
                                                 const scrappie_hip_squiggle_params *p, int viterbi, float *score) {
    if (ncand && (!cand || !score)) return set_err("squiggle_match_multi: null argument");
    std::fill(score, score + ncand, NAN);
    const scrappie_hip_squiggle_params dp = scrappie_hip_default_squiggle_params();
    if (squig_params_ok("squiggle_match_multi", p ? p : &dp)) return -1;
    if (ncand == 0) return 0;
    if (squig_signal_ok("squiggle_match_multi", signal)) return -1;
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    const scrappie_hip_squiggle_candidates cs = {cand, ncand};
    scrappie_hip_squiggle_multi_result res;
    if (scrappie_hip_squiggle_match_multi_batch(e, &signal, &cs, 1, p, viterbi, 0, &res)) return -1;
    if (res.score) memcpy(score, res.score, ncand * sizeof(float));
    scrappie_hip_free_squiggle_multi_results(&res, 1);
    return 0;
}
