/* sh_eng_crf_find.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * short sequences (motifs) searched INSIDE reads of a flip-flop (CRF) model (k_crf_find, sh_crf_find.h).  find_crf_sequences_viterbi
 * on the process-default engine (the caller's host matrix uploaded, the reference-layout loader) and scrappie_hip_find_batch: the
 * network and k_crf<true> of a launch group (run_staged to STOP_POST), every pack of every read of the group in ONE k_crf_find
 * launch on the transitions where k_crf left them in d_E, under the engine's lock; scores, positions and call scores back.  The
 * packing itself is host arithmetic in sh_host.c (scrappie_hip_crf_find_plan). */

#define SH_CRF_FIND_CELLS 512       /* cells a pack holds unless the debug option "crf_find_cells" says otherwise: two chunks of 256 threads; the fastest on 24 motifs of 40 bases with positions and on 96 of 24 (profiles/crf_find_rate.txt), 256 within 3 % of it */

/* launches of each k_crf_find form in this process: index (pos ? 2 : 0) | (tiled ? 1 : 0) */
static std::atomic<uint64_t> g_crf_find_forms[4];
extern "C" void scrappie_hip_crf_find_form_counts(uint64_t forms[4]) {
    for (int k = 0; k < 4; k++) if (forms) forms[k] = g_crf_find_forms[k].load(std::memory_order_relaxed);
}

static const char *const CRF_FIND_NO_FIT = "no occurrence fits the read (the motif has more bases than the read has entries)";

/* One cand array of a call as every read that points at it sees it: checked, packed and laid out as k_crf_find reads it, once. */
struct FindSet {
    const scrappie_hip_map_target *cand = nullptr;
    size_t n = 0;
    std::string why;                          /* why its first motif that cannot be searched cannot */
    struct Pack { size_t cell, at, ncell, nmotif; };      /* where its cell words and its motifs begin in cellw / packed */
    std::vector<Pack> packs;                  /* never empty: a set without a motif to search is one pack of the five U cells (the call score) */
    std::vector<int> cellw;
    std::vector<size_t> packed;               /* the motifs in pack order */
    size_t maxcell = 0;                       /* cells of its largest pack */
    size_t bytes = 0;                         /* device bytes a read of this set adds to a launch */
};

static size_t crf_find_cells(const scrappie_hip_engine *e) { return e->crf_find_cells < 0 ? (size_t)SH_CRF_FIND_CELLS : (size_t)e->crf_find_cells; }

static void find_set_build(FindSet &cs, const scrappie_hip_map_target *cand, size_t n, size_t pack_cells) {
    cs.cand = cand; cs.n = n;
    std::vector<size_t> good, len;
    auto bad = [&](size_t k, const std::string &text) { if (cs.why.empty()) cs.why = "motif " + std::to_string(k) + ": " + text; };
    const size_t maxc = scrappie_hip_crf_find_max_cells();
    for (size_t k = 0; k < n; k++) {
        const scrappie_hip_map_target &t = cand[k];
        if (t.poslow || t.poshigh) { bad(k, "bands are not part of this call"); continue; }
        if (!t.seq) { bad(k, "no sequence"); continue; }
        if (t.seqlen == 0) { bad(k, "an empty sequence"); continue; }
        if (t.seqlen > maxc - 9) { bad(k, "a sequence of " + std::to_string(t.seqlen) + " bases is too long for k_crf_find (" + std::to_string(maxc - 9) + " at most)"); continue; }
        size_t i = 0;
        while (i < t.seqlen && t.seq[i] >= 0 && t.seq[i] <= 3) i++;
        if (i < t.seqlen) { bad(k, "sequence code " + std::to_string(t.seq[i]) + " at " + std::to_string(i) + " is not a base (0..3)"); continue; }
        good.push_back(k); len.push_back(t.seqlen);
    }
    std::vector<int> pack(good.size(), -1);               /* (none stays -1: the planner's bound is the one checked above) */
    std::vector<long long> cell(good.size(), -1);
    const size_t np = good.empty() ? 0 : (size_t)scrappie_hip_crf_find_plan(len.data(), good.size(), pack_cells, pack.data(), cell.data());
    cs.packs.resize(std::max<size_t>(np, 1));
    auto open = [&](size_t p) {
        cs.packs[p] = FindSet::Pack{cs.cellw.size(), cs.packed.size(), 5, 0};
        for (int s = 0; s < 5; s++) cs.cellw.push_back(SH_CFD_WORD(0, SH_CFD_U, s, 0, 0));
    };
    if (np == 0) open(0);
    int cur = -1;
    for (size_t j = 0; j < good.size(); j++) {
        const scrappie_hip_map_target &t = cand[good[j]];
        if (pack[j] != cur) { cur = pack[j]; open((size_t)cur); }
        FindSet::Pack &P = cs.packs[(size_t)cur];
        const size_t L = t.seqlen;
        for (size_t p = 1; p < L; p++) cs.cellw.push_back(SH_CFD_WORD(0, p == 1 ? SH_CFD_B1 : SH_CFD_INT, 0, t.seq[p - 1], p >= 2 ? t.seq[p - 2] : 0));
        for (int s = 0; s < 5; s++) cs.cellw.push_back(SH_CFD_WORD(P.nmotif, L >= 2 ? SH_CFD_V : SH_CFD_V1, s, t.seq[L - 1], L >= 2 ? t.seq[L - 2] : 0));
        P.ncell += L + 4; P.nmotif++;
        cs.packed.push_back(good[j]);
    }
    for (const FindSet::Pack &P : cs.packs) cs.maxcell = std::max(cs.maxcell, P.ncell);
    cs.bytes = cs.cellw.size() * 4 + cs.packs.size() * (sizeof(ShCrfFindPack) + 4) + cs.packed.size() * 12 + 64;
}

/* one read of a launch: where its transitions are (as map_crf_plan_add takes them), its motifs, and where the results go ([cs->n] each, NAN / -1 already;
 * begin and end may be NULL) */
struct FindJob { long long trans; int lane; size_t nblock; const FindSet *cs; float *score; int32_t *begin, *end; float call; };

/* The results of jobs[] (under mu): every pack of every read as a workgroup of one k_crf_find launch -- a set's cell words uploaded once however many
 * reads point at it.  trans: d_E or the uploaded matrices.  t (may be NULL): t[0] += the kernel, t[1] += copies. */
static int find_run(scrappie_hip_engine *e, std::vector<FindJob> &jobs, const float *trans, bool tiled, bool pos, double *t) {
    if (jobs.empty()) return 0;
    hipStream_t s = e->stream;
    std::vector<ShCrfFindPack> pk;
    std::vector<int> cellw;
    std::map<const FindSet *, size_t> up;
    std::vector<size_t> out0(jobs.size(), 0), pack0(jobs.size(), 0);
    size_t nscore = 0, maxcell = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        const FindJob &job = jobs[j];
        const FindSet &cs = *job.cs;
        out0[j] = nscore; pack0[j] = pk.size();
        auto it = up.find(&cs);
        if (it == up.end()) {
            it = up.emplace(&cs, cellw.size()).first;
            cellw.insert(cellw.end(), cs.cellw.begin(), cs.cellw.end());
            maxcell = std::max(maxcell, cs.maxcell);
        }
        for (const FindSet::Pack &P : cs.packs) {
            ShCrfFindPack q{};
            q.trans = job.trans; q.lane = job.lane; q.nblock = (int)job.nblock;
            q.cell = (long long)(it->second + P.cell); q.out = (long long)(nscore + P.at); q.ncell = (int)P.ncell;
            pk.push_back(q);
        }
        nscore += cs.packed.size();
    }
    const size_t np = pk.size(), lds = sh_crf_find_lds_bytes(maxcell, pos);
    if (lds > SH_MAP_LDS) return set_err("crf_find: a pack of %zu bytes of LDS", lds);
    if (e->d_cfd_rd.ensure(np * sizeof(ShCrfFindPack)) || e->d_cfd_cell.ensure(cellw.size() * 4 + 16) || e->d_cfd_score.ensure(nscore * 4 + 16) ||
        e->d_cfd_pos.ensure(nscore * 8 + 16) || e->d_cfd_call.ensure(np * 4 + 16) || e->h_cfd.ensure(nscore * 12 + np * 4 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(e->d_cfd_rd.p, pk.data(), np * sizeof(ShCrfFindPack), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_cfd_cell.p, cellw.data(), cellw.size() * 4, hipMemcpyHostToDevice, s));
    ShCrfFindArgs a{};
    a.packs = e->d_cfd_rd.as<ShCrfFindPack>(); a.trans = trans; a.cells = e->d_cfd_cell.as<int>();
    a.score = e->d_cfd_score.as<float>(); a.pos = e->d_cfd_pos.as<int2>(); a.call = e->d_cfd_call.as<float>();
    const auto t0 = std::chrono::steady_clock::now();
    if (pick_bool([&](auto ps, auto tl) {
            using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
            g_crf_find_forms[(ps() ? 2 : 0) | (tl() ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
            return launch_k<k_crf_find<ps(), LD>>(dim3((unsigned)np), dim3(SH_MAP_NTH), lds, s, a);
        }, pos, tiled)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    const auto t1 = std::chrono::steady_clock::now();
    const float *hc = e->h_cfd.as<float>(), *hs = hc + np;
    const int2 *hp = (const int2 *)(hs + nscore + ((np + nscore) & 1));      /* 8-byte aligned */
    HIPCHK(hipMemcpyAsync((void *)hc, e->d_cfd_call.p, np * 4, hipMemcpyDeviceToHost, s));
    if (nscore) HIPCHK(hipMemcpyAsync((void *)hs, e->d_cfd_score.p, nscore * 4, hipMemcpyDeviceToHost, s));
    if (nscore && pos) HIPCHK(hipMemcpyAsync((void *)hp, e->d_cfd_pos.p, nscore * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    for (size_t j = 0; j < jobs.size(); j++) {
        FindJob &job = jobs[j];
        const FindSet &cs = *job.cs;
        job.call = hc[pack0[j]];
        for (size_t i = 0; i < cs.packed.size(); i++) {
            const size_t k = cs.packed[i];
            const float sc = hs[out0[j] + i];
            if (!(sc >= -SH_MAP_BIG / 2)) continue;          /* no occurrence fits: NAN and -1 stay */
            job.score[k] = sc;
            if (pos && job.begin) job.begin[k] = hp[out0[j] + i].x;
            if (pos && job.end) job.end[k] = hp[out0[j] + i].y;
        }
    }
    if (t) {
        t[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    return 0;
}

/* the first motif of a set that was searched and fits nowhere (NAN from the kernel's score), -1: none */
static long find_first_unfit(const FindSet &cs, const float *score) {
    long first = -1;
    for (size_t k : cs.packed)
        if (std::isnan(score[k]) && (first < 0 || (long)k < first)) first = (long)k;
    return first;
}

/* the highest finite score, the lowest index on a tie; -1: none */
static int find_best(const float *score, size_t n) {
    int best = -1;
    for (size_t k = 0; k < n; k++)
        if (std::isfinite(score[k]) && (best < 0 || score[k] > score[best])) best = (int)k;
    return best;
}

/* ------------------------------------------------------------------ */
/* per-read symbol                                                      */
/* ------------------------------------------------------------------ */
extern "C" int find_crf_sequences_viterbi(const_scrappie_matrix tr, const scrappie_hip_map_target *motif, size_t nmotif, float *score, int32_t *begin,
                                          int32_t *end, float *call_score) {
    const char *const fn = "find_crf_sequences_viterbi";
    if (call_score) *call_score = NAN;
    if (!tr || (nmotif && (!motif || !score))) return set_err("%s: null argument", fn);
    std::fill(score, score + nmotif, NAN);
    if (begin) std::fill(begin, begin + nmotif, -1);
    if (end) std::fill(end, end + nmotif, -1);
    if (!sh_crf_post_ok(tr)) return set_err("%s: not a transition matrix of 25 rows and at least one block", fn);
    if (tr->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, tr->nc);
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    FindSet cs;
    find_set_build(cs, motif, nmotif, crf_find_cells(e));
    DBuf &dtr = e->d_map_post;
    const size_t nfl = (tr->nc - 1) * tr->stride + 25;           /* as far as the last column's 25th float */
    if (dtr.ensure(nfl * 4)) return -1;
    if (hipMemcpyAsync(dtr.p, tr->data.f, nfl * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess) return set_err("%s: upload failed", fn);
    std::vector<FindJob> jobs{FindJob{0, (int)tr->stride, tr->nc, &cs, score, begin, end, NAN}};
    if (find_run(e, jobs, dtr.as<float>(), false, begin || end, nullptr)) {
        const std::string keep = g_err;
        (void)hipGetLastError();
        std::fill(score, score + nmotif, NAN);
        return set_err("%s", keep.c_str());
    }
    if (call_score) *call_score = jobs[0].call;
    const long unfit = find_first_unfit(cs, score);
    if (!cs.why.empty()) set_err("%s: %s", fn, cs.why.c_str());
    else if (unfit >= 0) set_err("%s: motif %ld: %s", fn, unfit, CRF_FIND_NO_FIT);
    return 0;
}

/* ------------------------------------------------------------------ */
/* batched                                                              */
/* ------------------------------------------------------------------ */
static void find_blank(scrappie_hip_find_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].score); free(r[i].begin); free(r[i].end); r[i] = scrappie_hip_find_result{nullptr, nullptr, nullptr, 0, NAN, -1, 0}; }
}
extern "C" void scrappie_hip_free_find_results(scrappie_hip_find_result *r, size_t n) { if (r) find_blank(r, n); }

/* one launch group: reads idx[] of the call, setof[r] the motifs of read r */
static int find_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const std::vector<const FindSet *> &setof, const std::vector<size_t> &idx,
                      const scrappie_hip_params *p, bool pos, scrappie_hip_find_result *out, LaunchCut<MapLoad> &cut) {
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const raw_table *> win;
    for (size_t r : idx) win.push_back(&reads[r]);
    RunOut ro;
    std::vector<unsigned> bad;
    if (run_staged(e, m, win, p, STOP_POST, 5, &ro, bad, e->map_ms)) return -1;
    const LaunchGroup &lg = e->current().lg;
    std::vector<FindJob> jobs;
    std::vector<size_t> who;
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0) continue;
        const size_t r = idx[(size_t)o];
        if (bad[i]) {
            cut.refuse(r, "the read holds values outside the supported range (is the signal trimmed and med/MAD-normalised?)");
            continue;
        }
        jobs.push_back(FindJob{lg.tile_boff[i >> 4], (int)(i & 15), (size_t)lg.rT[i], setof[r], out[r].score, out[r].begin, out[r].end, NAN});
        who.push_back(r);
    }
    if (find_run(e, jobs, ro.E, true, pos, e->map_ms + 1)) return -1;
    for (size_t j = 0; j < jobs.size(); j++) {
        scrappie_hip_find_result &res = out[who[j]];
        res.nblock = jobs[j].nblock;
        res.call_score = jobs[j].call;
        res.best = find_best(res.score, res.nmotif);
        const long unfit = find_first_unfit(*jobs[j].cs, res.score);
        if (unfit >= 0) cut.refuse(who[j], ("motif " + std::to_string(unfit) + ": " + CRF_FIND_NO_FIT).c_str());
    }
    return 0;
}

extern "C" int scrappie_hip_find_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *motifs, size_t n,
                                       const scrappie_hip_params *p, int want_pos, scrappie_hip_find_result *out) {
    if (!e || (n && (!reads || !motifs || !out))) return set_err("find_batch: null argument");
    std::lock_guard<std::mutex> call(e->call_mu);
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_find_result{nullptr, nullptr, nullptr, 0, NAN, -1, 0};
    Model *m = get_model(e, model);
    if (!m) return -1;
    if (m->arch != 1) return set_err("find_batch: model '%s' is a transducer model; sequences are searched inside reads of flip-flop (CRF) models only", m->name.c_str());
    scrappie_hip_params dp = scrappie_hip_default_params();
    if (!p) p = &dp;
    (void)hipSetDevice(e->device);
    for (double &x : e->map_ms) x = 0.0;
    const bool pos = want_pos != 0;
    /* the motifs: one set per distinct cand array of the call */
    std::map<std::pair<const scrappie_hip_map_target *, size_t>, std::unique_ptr<FindSet>> sets;
    std::vector<const FindSet *> setof(n, nullptr);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = motifs[i].cand ? motifs[i].ncand : 0;
        out[i].score = (float *)malloc(std::max<size_t>(nc, 1) * sizeof(float));
        if (pos) { out[i].begin = (int32_t *)malloc(std::max<size_t>(nc, 1) * 4); out[i].end = (int32_t *)malloc(std::max<size_t>(nc, 1) * 4); }
        if (!out[i].score || (pos && (!out[i].begin || !out[i].end))) { find_blank(out, n); return set_err("find_batch: out of host memory"); }
        std::fill(out[i].score, out[i].score + nc, NAN);
        if (pos) { std::fill(out[i].begin, out[i].begin + nc, -1); std::fill(out[i].end, out[i].end + nc, -1); }
        out[i].nmotif = nc;
        std::unique_ptr<FindSet> &cs = sets[std::make_pair(nc ? motifs[i].cand : nullptr, nc)];
        if (!cs) { cs.reset(new FindSet()); find_set_build(*cs, motifs[i].cand, nc, crf_find_cells(e)); }
        setof[i] = cs.get();
    }
    /* launch groups as scrappie_hip_map_batch cuts them; a read adds its cell words, packs and results */
    const size_t bpb = bytes_per_block(m, true);
    const size_t budget = e->max_launch_blocks ? e->max_launch_blocks * bpb : (size_t)(e->mem_frac * (double)e->total_mem);
    auto cost = [&](size_t sT, size_t mT, size_t ex) { return (sT / 16 + mT + 1) * bpb + ex; };
    LaunchCut<MapLoad> cut{e, "find_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) { return find_group(e, m, reads, setof, grp, p, pos, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (motifs[i].ncand && !motifs[i].cand) cut.refuse(i, "no motifs");
        const size_t T = map_blocks(m, map_read_nsample(m, reads[i]));
        if (T == 0) { cut.refuse(i, "read too short for the model (or empty)"); continue; }
        if (T > (size_t)INT32_MAX / 2) { cut.refuse(i, "too many blocks"); continue; }
        const FindSet *cs = setof[i];
        if (!cs->why.empty()) cut.refuse(i, cs->why.c_str());      /* (its other motifs are searched) */
        const size_t rb = cs->bytes;
        if (cost(T, T, rb) > budget) { cut.refuse(i, "read and motifs too long for one launch group on this device"); continue; }
        MapLoad &g = cut.load;
        cut.add(i, cut.who.size() < e->max_launch_reads && cost(g.sumT + T, std::max(g.maxT, T), g.extra + rb) <= budget);
        cut.load.sumT += T; cut.load.maxT = std::max(cut.load.maxT, T); cut.load.extra += rb;
    }
    return cut.finish([&] { find_blank(out, n); },
                      [](size_t i, const char *why) { set_err("find_batch: read %zu: %s", i, why); });
}
