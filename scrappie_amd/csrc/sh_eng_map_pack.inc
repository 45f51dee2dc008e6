/* sh_eng_map_pack.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * one read against many candidate sequences (k_map_pack, sh_map_pack.h).  scrappie_hip_map_multi_batch: the network and S1 of a
 * launch group ONCE (run_staged to STOP_POST, as map_group), every read's candidates packed end to end into workgroups of one
 * k_map_pack launch on the posterior where S1 left it, the candidates too long for a pack through k_map (plan_add + map_run) on
 * the same posterior, scores back; with a path wanted, a second pass of k_map on each read's best candidate alone while the
 * posterior is still resident.  scrappie_hip_map_post_multi: the same on a host posterior and the process-default engine.
 * The packing itself is host arithmetic in sh_host.c (scrappie_hip_map_pack_plan). */

#define SH_MAP_PACK_CELLS 256       /* cells a pack holds unless the debug option "map_pack_cells" says otherwise: the fastest on 24 barcodes of 40 bases, faster than k_map per candidate on 8 x 400 bases (profiles/map_multi_rate.txt) */

/* launches of each k_map_pack form in this process: index (vit ? 2 : 0) | (tiled ? 1 : 0) */
static std::atomic<uint64_t> g_map_pack_forms[4];
extern "C" void scrappie_hip_map_pack_form_counts(uint64_t forms[4]) {
    for (int k = 0; k < 4; k++) if (forms) forms[k] = g_map_pack_forms[k].load(std::memory_order_relaxed);
}

/* One cand array of a call as every read that points at it sees it: checked, packed and laid out as k_map_pack reads it, once. */
struct MapCandSet {
    const scrappie_hip_map_target *cand = nullptr;
    size_t n = 0;
    std::string why;                          /* why its first candidate that cannot be mapped cannot */
    struct Pack { size_t cell, first, at, ncell, ncand; };       /* where its cell words, its first cells and its candidates begin in cellw / firsts / packed */
    std::vector<Pack> packs;
    std::vector<int> cellw, firsts;
    std::vector<size_t> packed, over;         /* the candidates in pack order; those that take k_map */
    size_t maxL = 0;                          /* the longest candidate that can be mapped */
    size_t lds = 0;                           /* dynamic LDS of its largest pack */
    size_t bytes = 0;                         /* device bytes a read of this set adds to a launch, a path's second pass apart */
};

/* nr: posterior rows; nblock: of the read where it is known (else 1: the caller checks its reads); pack_cells 0: every candidate through k_map */
static void map_cand_set_build(MapCandSet &cs, const char *fn, const scrappie_hip_map_target *cand, size_t n, size_t nr, size_t nblock, size_t pack_cells) {
    cs.cand = cand; cs.n = n;
    std::vector<size_t> good, len;
    const std::string pre = std::string(fn) + ": ";
    auto bad = [&](size_t k, const char *text) {        /* (map_target_ok's texts begin with fn, as the caller's own will) */
        if (cs.why.empty()) cs.why = "candidate " + std::to_string(k) + ": " + (strncmp(text, pre.c_str(), pre.size()) ? text : text + pre.size());
    };
    for (size_t k = 0; k < n; k++) {
        const scrappie_hip_map_target &t = cand[k];
        if (t.poslow || t.poshigh) { bad(k, "bands are not part of this call"); continue; }
        if (!t.seq) { bad(k, "no sequence"); continue; }
        if (map_target_ok(fn, nr, nblock, t.seq, t.seqlen, nullptr, nullptr, false)) { bad(k, g_err); continue; }
        good.push_back(k); len.push_back(t.seqlen);
        cs.maxL = std::max(cs.maxL, t.seqlen);
    }
    std::vector<int> pack(good.size(), -1);
    std::vector<long long> cell(good.size(), -1);
    if (pack_cells && !good.empty()) cs.packs.resize((size_t)scrappie_hip_map_pack_plan(len.data(), good.size(), pack_cells, pack.data(), cell.data()));
    int cur = -1;
    auto close = [&] {
        if (cur < 0) return;
        const MapCandSet::Pack &P = cs.packs[(size_t)cur];
        cs.firsts.push_back((int)P.ncell);
        cs.lds = std::max(cs.lds, sh_map_pack_lds_bytes(P.ncell, P.ncand));
    };
    for (size_t j = 0; j < good.size(); j++) {
        const scrappie_hip_map_target &t = cand[good[j]];
        if (pack[j] < 0) { cs.over.push_back(good[j]); cs.bytes += map_read_bytes(t.seqlen, 1, false, false); continue; }
        if (pack[j] != cur) { close(); cur = pack[j]; cs.packs[(size_t)cur] = MapCandSet::Pack{cs.cellw.size(), cs.firsts.size(), cs.packed.size(), 0, 0}; }
        MapCandSet::Pack &P = cs.packs[(size_t)cur];
        cs.firsts.push_back((int)P.ncell);
        cs.cellw.push_back(SH_MPK_START << SH_MPK_KIND_SHIFT);
        for (size_t i = 0; i < t.seqlen; i++) cs.cellw.push_back(((i == 0 ? SH_MPK_POS0 : i == 1 ? SH_MPK_POS1 : SH_MPK_POS2) << SH_MPK_KIND_SHIFT) | t.seq[i]);
        cs.cellw.push_back(SH_MPK_END << SH_MPK_KIND_SHIFT);
        P.ncell += t.seqlen + 2; P.ncand++;
        cs.packed.push_back(good[j]);
    }
    close();
    cs.bytes += (cs.cellw.size() + cs.firsts.size() + n) * 4 + cs.packs.size() * sizeof(ShMapPack) + 64;
}

/* the state codes share a cell word with the cell's kind */
static int map_pack_states_ok(const char *fn, size_t nr) {
    return nr > (size_t)SH_MPK_CODE_MASK ? set_err("%s: a posterior of %zu states is more than a pack's cell words hold", fn, nr) : 0;
}

static size_t map_pack_cells(const scrappie_hip_engine *e) { return e->map_pack_cells < 0 ? (size_t)SH_MAP_PACK_CELLS : (size_t)e->map_pack_cells; }

/* one read of a launch: where its posterior is (as plan_add takes it), its candidates, and where their scores go ([cs->n], NAN already) */
struct MapMultiJob { long long post; int lane; size_t nblock; const MapCandSet *cs; float *score; };

/* The scores of jobs[] (under mu): every pack of every read as a workgroup of one k_map_pack launch -- a set's tables uploaded once however
 * many reads point at it --, the candidates left to k_map as one map_run.  a: the posterior, its shape and the penalties.
 * t (may be NULL): t[0] += the kernels, t[1] += copies. */
static int map_multi_run(scrappie_hip_engine *e, const std::vector<MapMultiJob> &jobs, ShMapArgs a, bool vit, bool tiled, double *t) {
    hipStream_t s = e->stream;
    std::vector<ShMapPack> pk;
    std::vector<int> cellw, firsts;
    std::map<const MapCandSet *, std::pair<size_t, size_t>> up;
    std::vector<size_t> out0(jobs.size(), 0);
    size_t nscore = 0, lds = 0;
    MapPlan over;
    std::vector<std::pair<size_t, size_t>> over_who;          /* (job, candidate) */
    for (size_t j = 0; j < jobs.size(); j++) {
        const MapMultiJob &job = jobs[j];
        const MapCandSet &cs = *job.cs;
        out0[j] = nscore;
        if (!cs.packs.empty()) {
            auto it = up.find(&cs);
            if (it == up.end()) {
                it = up.emplace(&cs, std::make_pair(cellw.size(), firsts.size())).first;
                cellw.insert(cellw.end(), cs.cellw.begin(), cs.cellw.end());
                firsts.insert(firsts.end(), cs.firsts.begin(), cs.firsts.end());
                lds = std::max(lds, cs.lds);
            }
            for (const MapCandSet::Pack &P : cs.packs) {
                ShMapPack q{};
                q.post = job.post; q.lane = job.lane; q.nblock = (int)job.nblock;
                q.cell = (long long)(it->second.first + P.cell); q.first = (long long)(it->second.second + P.first);
                q.out = (long long)(nscore + P.at); q.ncell = (int)P.ncell; q.ncand = (int)P.ncand;
                pk.push_back(q);
            }
            nscore += cs.packed.size();
        }
        for (size_t k : cs.over) {
            plan_add(over, job.post, job.lane, job.nblock, cs.cand[k].seq, cs.cand[k].seqlen, nullptr, nullptr, false);
            over_who.emplace_back(j, k);
        }
    }
    if (!pk.empty()) {
        if (lds > SH_MAP_LDS) return set_err("map_multi: a pack of %zu bytes of LDS", lds);
        if (e->d_mpk_rd.ensure(pk.size() * sizeof(ShMapPack)) || e->d_mpk_cell.ensure(cellw.size() * 4 + 16) || e->d_mpk_first.ensure(firsts.size() * 4 + 16) ||
            e->d_mpk_score.ensure(nscore * 4 + 16) || e->h_mpk.ensure(nscore * 4 + 16)) return -1;
        HIPCHK(hipMemcpyAsync(e->d_mpk_rd.p, pk.data(), pk.size() * sizeof(ShMapPack), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e->d_mpk_cell.p, cellw.data(), cellw.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e->d_mpk_first.p, firsts.data(), firsts.size() * 4, hipMemcpyHostToDevice, s));
        a.score = e->d_mpk_score.as<float>();
        const auto t0 = std::chrono::steady_clock::now();
        if (pick_bool([&](auto v, auto tl) {
                g_map_pack_forms[(v() ? 2 : 0) | (tl() ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
                return launch_k<k_map_pack<v(), tl()>>(dim3((unsigned)pk.size()), dim3(SH_MAP_NTH), lds, s, a, (const ShMapPack *)e->d_mpk_rd.p,
                                                       (const int *)e->d_mpk_cell.p, (const int *)e->d_mpk_first.p);
            }, vit, tiled)) return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(sh_stream_wait(s));
        const auto t1 = std::chrono::steady_clock::now();
        const float *hs = e->h_mpk.as<float>();
        HIPCHK(hipMemcpyAsync(e->h_mpk.p, e->d_mpk_score.p, nscore * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
        for (size_t j = 0; j < jobs.size(); j++) {
            const MapCandSet &cs = *jobs[j].cs;
            if (cs.packs.empty()) continue;
            for (size_t i = 0; i < cs.packed.size(); i++) jobs[j].score[cs.packed[i]] = hs[out0[j] + i];
        }
        if (t) {
            t[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
            t[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        }
    }
    if (!over_who.empty()) {
        std::vector<float> sc(over_who.size(), NAN);
        if (map_run(e, over, a, vit, false, tiled, sc.data(), nullptr, t)) return -1;
        for (size_t i = 0; i < over_who.size(); i++) jobs[over_who[i].first].score[over_who[i].second] = sc[i];
    }
    return 0;
}

/* the highest finite score, the lowest index on a tie; -1: none */
static int map_multi_best(const float *score, size_t n) {
    int best = -1;
    for (size_t k = 0; k < n; k++)
        if (std::isfinite(score[k]) && (best < 0 || score[k] > score[best])) best = (int)k;
    return best;
}

static void map_multi_blank(scrappie_hip_map_multi_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].score); free(r[i].path); r[i] = scrappie_hip_map_multi_result{nullptr, 0, -1, 0, nullptr}; }
}
extern "C" void scrappie_hip_free_map_multi_results(scrappie_hip_map_multi_result *r, size_t n) { if (r) map_multi_blank(r, n); }

/* one launch group: reads idx[0..cnt) of the call, setof[r] the candidates of read r */
static int map_multi_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const std::vector<const MapCandSet *> &setof, const std::vector<size_t> &idx,
                           const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_multi_result *out, LaunchCut<MapLoad> &cut) {
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const raw_table *> win;
    for (size_t r : idx) win.push_back(&reads[r]);
    RunOut ro;
    std::vector<unsigned> bad;
    if (run_staged(e, m, win, p, STOP_POST, 5, &ro, bad, e->map_ms)) return -1;
    const LaunchGroup &lg = e->current().lg;
    std::vector<MapMultiJob> jobs;
    std::vector<size_t> who;
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0) continue;
        const size_t r = idx[(size_t)o];
        if (bad[i]) {
            cut.refuse(r, "the read holds values outside the supported range (is the signal trimmed and med/MAD-normalised?)");
            continue;
        }
        jobs.push_back(MapMultiJob{lg.tile_boff[i >> 4], (int)(i & 15), (size_t)lg.rT[i], setof[r], out[r].score});
        who.push_back(r);
    }
    ShMapArgs a{};
    a.E = ro.E; a.sums = ro.sums; a.nr = m->NS; a.nchunk = m->ff_mtiles; a.min_prob = p->min_prob;
    a.stay_pen = p->stay_pen; a.skip_pen = p->skip_pen; a.local_pen = p->local_pen;
    if (map_multi_run(e, jobs, a, vit, true, e->map_ms + 1)) return -1;
    MapPlan second;                        /* each read's best candidate alone, with its traceback: before anything can overwrite d_E */
    std::vector<size_t> second_who;
    for (size_t j = 0; j < jobs.size(); j++) {
        scrappie_hip_map_multi_result &res = out[who[j]];
        res.nblock = jobs[j].nblock;
        res.best = map_multi_best(res.score, res.ncand);
        if (!(vit && want_path) || res.best < 0) continue;
        const scrappie_hip_map_target &t = jobs[j].cs->cand[res.best];
        plan_add(second, jobs[j].post, jobs[j].lane, jobs[j].nblock, t.seq, t.seqlen, nullptr, nullptr, true);
        second_who.push_back(who[j]);
    }
    if (!second_who.empty()) {
        std::vector<float> sc(second_who.size(), NAN);
        std::vector<int32_t *> paths(second_who.size(), nullptr);
        if (map_run(e, second, a, true, false, true, sc.data(), paths.data(), e->map_ms + 1)) {
            for (int32_t *q : paths) free(q);
            return -1;
        }
        for (size_t k = 0; k < second_who.size(); k++) out[second_who[k]].path = paths[k];
    }
    return 0;
}

extern "C" int scrappie_hip_map_multi_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *cands,
                                            size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_multi_result *out) {
    if (!e || (n && (!reads || !cands || !out))) return set_err("map_multi_batch: null argument");
    std::lock_guard<std::mutex> call(e->call_mu);
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_map_multi_result{nullptr, 0, -1, 0, nullptr};
    Model *m = get_model(e, model);
    if (!m) return -1;
    if (m->arch == 1) return set_err("map_multi_batch: model '%s' is a flip-flop (CRF) model; candidates are mapped with transducer models only", m->name.c_str());
    int nk = m->NS - 1;
    while (nk > 1 && nk % 4 == 0) nk /= 4;
    if (nk != 1) return set_err("map_multi_batch: model '%s' has %d states, not 4^k + 1", m->name.c_str(), m->NS);
    if (map_pack_states_ok("map_multi_batch", (size_t)m->NS)) return -1;
    scrappie_hip_params dp = scrappie_hip_default_params();
    if (!p) p = &dp;
    (void)hipSetDevice(e->device);
    for (double &x : e->map_ms) x = 0.0;
    const bool vit = viterbi != 0, wp = want_path != 0;
    /* the candidates: one set per distinct cand array of the call */
    std::map<std::pair<const scrappie_hip_map_target *, size_t>, std::unique_ptr<MapCandSet>> sets;
    std::vector<const MapCandSet *> setof(n, nullptr);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = cands[i].ncand;
        out[i].score = (float *)malloc(std::max<size_t>(nc, 1) * sizeof(float));
        if (!out[i].score) { map_multi_blank(out, n); return set_err("map_multi_batch: out of host memory"); }
        std::fill(out[i].score, out[i].score + nc, NAN);
        out[i].ncand = nc;
        if (!nc || !cands[i].cand) continue;
        std::unique_ptr<MapCandSet> &cs = sets[std::make_pair(cands[i].cand, nc)];
        if (!cs) { cs.reset(new MapCandSet()); map_cand_set_build(*cs, "map_multi_batch", cands[i].cand, nc, (size_t)m->NS, 1, map_pack_cells(e)); }
        setof[i] = cs.get();
    }
    /* launch groups as scrappie_hip_map_batch cuts them; a read adds its tables and scores, the rows of the candidates left to k_map and, with a
     * path, the second pass on its longest candidate */
    const size_t bpb = bytes_per_block(m, true);
    const size_t budget = e->max_launch_blocks ? e->max_launch_blocks * bpb : (size_t)(e->mem_frac * (double)e->total_mem);
    auto cost = [&](size_t sT, size_t mT, size_t ex) { return (sT / 16 + mT + 1) * bpb + ex; };
    LaunchCut<MapLoad> cut{e, "map_multi_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) { return map_multi_group(e, m, reads, setof, grp, p, vit, wp, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (cands[i].ncand && !cands[i].cand) { cut.refuse(i, "no candidates"); continue; }
        const size_t T = map_blocks(m, map_read_nsample(m, reads[i]));
        if (T == 0) { cut.refuse(i, "read too short for the model (or empty)"); continue; }
        if (T > (size_t)INT32_MAX / 2) { cut.refuse(i, "too many blocks"); continue; }
        const MapCandSet *cs = setof[i];
        if (!cs) { out[i].nblock = T; continue; }                  /* no candidates: a read with no scores */
        if (!cs->why.empty()) cut.refuse(i, cs->why.c_str());      /* (its other candidates are scored) */
        if (cs->packed.empty() && cs->over.empty()) { out[i].nblock = T; continue; }
        const size_t rb = cs->bytes + (vit && wp ? map_read_bytes(cs->maxL, T, false, true) : 0);
        if (cost(T, T, rb) > budget) { cut.refuse(i, "read and candidates too long for one launch group on this device"); continue; }
        MapLoad &g = cut.load;
        cut.add(i, cut.who.size() < e->max_launch_reads && cost(g.sumT + T, std::max(g.maxT, T), g.extra + rb) <= budget);
        g.sumT += T; g.maxT = std::max(g.maxT, T); g.extra += rb;
    }
    return cut.finish([&] { map_multi_blank(out, n); },
                      [](size_t i, const char *why) { set_err("map_multi_batch: read %zu: %s", i, why); });
}

extern "C" int scrappie_hip_map_post_multi(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                           const scrappie_hip_map_target *cand, size_t ncand, int viterbi, float *score) {
    if (!logpost || (ncand && (!cand || !score))) return set_err("map_post_multi: null argument");
    std::fill(score, score + ncand, NAN);
    if (ncand == 0) return 0;
    if (map_pack_states_ok("map_post_multi", logpost->nr)) return -1;
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    MapCandSet cs;
    map_cand_set_build(cs, "map_post_multi", cand, ncand, logpost->nr, logpost->nc, map_pack_cells(e));
    if (!cs.packed.empty() || !cs.over.empty()) {
        DBuf &dpost = e->d_map_post;
        const size_t pbytes = logpost->nc * logpost->stride * 4;
        if (dpost.ensure(pbytes)) return -1;
        HIPCHK(hipMemcpyAsync(dpost.p, logpost->data.f, pbytes, hipMemcpyHostToDevice, e->stream));
        ShMapArgs a{};
        a.post = dpost.as<float>(); a.pstride = (long long)logpost->stride; a.nr = (int)logpost->nr;
        a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
        const std::vector<MapMultiJob> jobs{MapMultiJob{0, 0, logpost->nc, &cs, score}};
        if (map_multi_run(e, jobs, a, viterbi != 0, false, nullptr)) {
            const std::string keep = g_err;
            (void)hipGetLastError();
            std::fill(score, score + ncand, NAN);
            return set_err("%s", keep.c_str());
        }
    }
    if (!cs.why.empty()) set_err("map_post_multi: %s", cs.why.c_str());
    return 0;
}
