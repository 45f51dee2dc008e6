/* sh_eng_map_pack.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * one read against many candidate sequences (k_map_pack, sh_map_pack.h).  scrappie_hip_map_multi_batch: the network and S1 of a
 * launch group ONCE (run_staged to STOP_POST, as map_group), every read's candidates packed end to end into workgroups of one
 * k_map_pack launch on the posterior where S1 left it, the candidates too long for a pack through k_map (plan_add + dp_run) on
 * the same posterior, scores back; with a path wanted, a second pass of k_map on each read's best candidate alone while the
 * posterior is still resident.  scrappie_hip_map_post_multi: the same on a host posterior and the process-default engine.
 * The packing itself is host arithmetic in sh_host.c (scrappie_hip_map_pack_plan).  What is here is the family's own: how a candidate becomes
 * cell words, the pack record, the launch, the second pass.  Sets, their registry, the layout of a launch and the scatter of its scores, the
 * batch call and the launch group's stage are sh_eng_post.inc's. */

#define SH_MAP_PACK_CELLS 256       /* cells a pack holds unless the debug option "map_pack_cells" says otherwise: the fastest on 24 barcodes of 40 bases, faster than k_map per candidate on 8 x 400 bases (profiles/map_multi_rate.txt) */

/* launches of each k_map_pack form in this process: index (vit ? 2 : 0) | (tiled ? 1 : 0) */
static std::atomic<uint64_t> g_map_pack_forms[4];
extern "C" void scrappie_hip_map_pack_form_counts(uint64_t forms[4]) {
    for (int k = 0; k < 4; k++) if (forms) forms[k] = g_map_pack_forms[k].load(std::memory_order_relaxed);
}

/* a PackSet (sh_eng_post.inc) of candidates as k_map_pack reads them */
struct MapCandSet : PackSet {
    std::vector<size_t> over;                 /* the candidates that take k_map */
    size_t maxL = 0;                          /* the longest candidate that can be mapped */
    size_t lds = 0;                           /* dynamic LDS of its largest pack */
};                                            /* (bytes: a path's second pass apart) */

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
        const PackSet::Pack &P = cs.packs[(size_t)cur];
        cs.firsts.push_back((int)P.ncell);
        cs.lds = std::max(cs.lds, sh_map_pack_lds_bytes(P.ncell, P.nitem));
    };
    for (size_t j = 0; j < good.size(); j++) {
        const scrappie_hip_map_target &t = cand[good[j]];
        if (pack[j] < 0) { cs.over.push_back(good[j]); cs.bytes += map_read_bytes(t.seqlen, 1, false, false); continue; }
        if (pack[j] != cur) { close(); cur = pack[j]; cs.packs[(size_t)cur] = PackSet::Pack{cs.cellw.size(), cs.firsts.size(), cs.packed.size(), 0, 0}; }
        PackSet::Pack &P = cs.packs[(size_t)cur];
        cs.firsts.push_back((int)P.ncell);
        cs.cellw.push_back(SH_MPK_START << SH_MPK_KIND_SHIFT);
        for (size_t i = 0; i < t.seqlen; i++) cs.cellw.push_back(((i == 0 ? SH_MPK_POS0 : i == 1 ? SH_MPK_POS1 : SH_MPK_POS2) << SH_MPK_KIND_SHIFT) | t.seq[i]);
        cs.cellw.push_back(SH_MPK_END << SH_MPK_KIND_SHIFT);
        P.ncell += t.seqlen + 2; P.nitem++;
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

/* The scores of jobs[] (under mu): every pack of every read as a workgroup of one k_map_pack launch (PackLaunch, sh_eng_post.inc), the candidates
 * left to k_map as one dp_run.  a: the posterior, its shape and the penalties.  t (may be NULL): t[0] += the kernels, t[1] += copies. */
static int map_multi_run(scrappie_hip_engine *e, const std::vector<MapMultiJob> &jobs, ShMapArgs a, bool vit, bool tiled, double *t) {
    hipStream_t s = e->stream;
    std::vector<ShMapPack> pk;
    PackLaunch<MapCandSet> L;
    L.lay(jobs, [&](size_t j, const PackSet::Pack &P, size_t cell, size_t first, size_t out) {
        ShMapPack q{};
        q.post = jobs[j].post; q.lane = jobs[j].lane; q.nblock = (int)jobs[j].nblock;
        q.cell = (long long)cell; q.first = (long long)first; q.out = (long long)out; q.ncell = (int)P.ncell; q.ncand = (int)P.nitem;
        pk.push_back(q);
    });
    MapPlan over;
    std::vector<std::pair<size_t, size_t>> over_who;          /* (job, candidate) */
    for (size_t j = 0; j < jobs.size(); j++)
        for (size_t k : jobs[j].cs->over) {
            const scrappie_hip_map_target &c = jobs[j].cs->cand[k];
            plan_add(over, jobs[j].post, jobs[j].lane, jobs[j].nblock, c.seq, c.seqlen, nullptr, nullptr, false);
            over_who.emplace_back(j, k);
        }
    if (!pk.empty()) {
        size_t lds = 0;
        for (const auto &kv : L.up) lds = std::max(lds, kv.first->lds);
        const size_t nscore = L.nscore;
        if (lds > SH_MAP_LDS) return set_err("map_multi: a pack of %zu bytes of LDS", lds);
        if (e->d_mpk_rd.ensure(pk.size() * sizeof(ShMapPack)) || e->d_mpk_cell.ensure(L.cellw.size() * 4 + 16) || e->d_mpk_first.ensure(L.firsts.size() * 4 + 16) ||
            e->d_mpk_score.ensure(nscore * 4 + 16) || e->h_mpk.ensure(nscore * 4 + 16)) return -1;
        HIPCHK(hipMemcpyAsync(e->d_mpk_rd.p, pk.data(), pk.size() * sizeof(ShMapPack), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e->d_mpk_cell.p, L.cellw.data(), L.cellw.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e->d_mpk_first.p, L.firsts.data(), L.firsts.size() * 4, hipMemcpyHostToDevice, s));
        a.score = e->d_mpk_score.as<float>();
        Span2 span;
        if (pick_bool([&](auto v, auto tl) {
                g_map_pack_forms[(v() ? 2 : 0) | (tl() ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
                return launch_k<k_map_pack<v(), tl()>>(dim3((unsigned)pk.size()), dim3(SH_MAP_NTH), lds, s, a, (const ShMapPack *)e->d_mpk_rd.p,
                                                       (const int *)e->d_mpk_cell.p, (const int *)e->d_mpk_first.p);
            }, vit, tiled)) return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(sh_stream_wait(s));
        span.mark();
        const float *hs = e->h_mpk.as<float>();
        HIPCHK(hipMemcpyAsync(e->h_mpk.p, e->d_mpk_score.p, nscore * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
        L.scatter(jobs, [&](const MapMultiJob &job, size_t k, size_t slot) { job.score[k] = hs[slot]; });
        span.add(t);
    }
    if (!over_who.empty()) {
        std::vector<float> sc(over_who.size(), NAN);
        if (dp_run(e, over, a, vit, false, tiled, sc.data(), nullptr, t)) return -1;
        for (size_t i = 0; i < over_who.size(); i++) jobs[over_who[i].first].score[over_who[i].second] = sc[i];
    }
    return 0;
}

static void map_multi_blank(scrappie_hip_map_multi_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].score); free(r[i].path); r[i] = scrappie_hip_map_multi_result{nullptr, 0, -1, 0, nullptr}; }
}
extern "C" void scrappie_hip_free_map_multi_results(scrappie_hip_map_multi_result *r, size_t n) { if (r) map_multi_blank(r, n); }

/* one launch group: reads idx[] of the call (post_group, sh_eng_post.inc), setof[r] the candidates of read r */
static int map_multi_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const std::vector<const MapCandSet *> &setof, const std::vector<size_t> &idx,
                           const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_multi_result *out, LaunchCut<MapLoad> &cut) {
    return post_group(e, m, reads, idx, p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
        std::vector<MapMultiJob> jobs;
        for (const PostRead &q : rd) jobs.push_back(MapMultiJob{q.boff, q.lane, q.nblock, setof[q.r], out[q.r].score});
        const ShMapArgs a = map_group_args(m, p, ro);
        if (map_multi_run(e, jobs, a, vit, true, e->map_ms + 1)) return -1;
        MapPlan second;                        /* each read's best candidate alone, with its traceback: before anything can overwrite d_E */
        std::vector<size_t> second_who;
        for (size_t j = 0; j < jobs.size(); j++) {
            scrappie_hip_map_multi_result &res = out[rd[j].r];
            res.nblock = jobs[j].nblock;
            res.best = best_finite(res.score, res.ncand);
            if (!(vit && want_path) || res.best < 0) continue;
            const scrappie_hip_map_target &t = jobs[j].cs->cand[res.best];
            plan_add(second, jobs[j].post, jobs[j].lane, jobs[j].nblock, t.seq, t.seqlen, nullptr, nullptr, true);
            second_who.push_back(rd[j].r);
        }
        if (!second_who.empty()) {
            std::vector<float> sc(second_who.size(), NAN);
            std::vector<int32_t *> paths(second_who.size(), nullptr);
            if (dp_run(e, second, a, true, false, true, sc.data(), paths.data(), e->map_ms + 1)) {
                for (int32_t *q : paths) free(q);
                return -1;
            }
            for (size_t k = 0; k < second_who.size(); k++) out[second_who[k]].path = paths[k];
        }
        return 0;
    });
}

extern "C" int scrappie_hip_map_multi_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *cands,
                                            size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_multi_result *out) {
    PostCall c(e, "map_multi_batch");
    if (c.enter(!n || (reads && cands && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_map_multi_result{nullptr, 0, -1, 0, nullptr};
    if (c.open(model, p, [](Model *m) {
            if (m->arch == 1) return set_err("map_multi_batch: model '%s' is a flip-flop (CRF) model; candidates are mapped with transducer models only", m->name.c_str());
            int nk = m->NS - 1;
            while (nk > 1 && nk % 4 == 0) nk /= 4;
            if (nk != 1) return set_err("map_multi_batch: model '%s' has %d states, not 4^k + 1", m->name.c_str(), m->NS);
            return map_pack_states_ok("map_multi_batch", (size_t)m->NS);
        })) return -1;
    Model *m = c.m;
    const bool vit = viterbi != 0, wp = want_path != 0;
    /* the candidates: one set per distinct cand array of the call */
    PackSets<MapCandSet> sets;
    std::vector<const MapCandSet *> &setof = sets.of;
    setof.assign(n, nullptr);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = cands[i].ncand;
        out[i].score = (float *)malloc(std::max<size_t>(nc, 1) * sizeof(float));
        if (!out[i].score) { map_multi_blank(out, n); return set_err("map_multi_batch: out of host memory"); }
        std::fill(out[i].score, out[i].score + nc, NAN);
        out[i].ncand = nc;
        if (!nc || !cands[i].cand) continue;
        setof[i] = sets.get(cands[i].cand, nc, [&](MapCandSet &cs) { map_cand_set_build(cs, "map_multi_batch", cands[i].cand, nc, (size_t)m->NS, 1, map_pack_cells(e)); });
    }
    /* launch groups as scrappie_hip_map_batch cuts them; a read adds its tables and scores, the rows of the candidates left to k_map and, with a
     * path, the second pass on its longest candidate */
    LaunchCut<MapLoad> cut{e, "map_multi_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) { return map_multi_group(e, m, reads, setof, grp, c.p, vit, wp, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (cands[i].ncand && !cands[i].cand) { cut.refuse(i, "no candidates"); continue; }
        const size_t T = c.blocks(cut, i, reads[i]);
        if (T == 0) continue;
        const MapCandSet *cs = setof[i];
        if (!cs) { out[i].nblock = T; continue; }                  /* no candidates: a read with no scores */
        if (!cs->why.empty()) cut.refuse(i, cs->why.c_str());      /* (its other candidates are scored) */
        if (cs->packed.empty() && cs->over.empty()) { out[i].nblock = T; continue; }
        c.add(cut, i, T, cs->bytes + (vit && wp ? map_read_bytes(cs->maxL, T, false, true) : 0),
              "read and candidates too long for one launch group on this device");
    }
    return c.finish(cut, [&] { map_multi_blank(out, n); });
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
        ShMapArgs a{};
        a.post = post_upload_dense(e, "map_post_multi", logpost);
        if (!a.post) return -1;
        a.pstride = (long long)logpost->stride; a.nr = (int)logpost->nr;
        a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
        const std::vector<MapMultiJob> jobs{MapMultiJob{0, 0, logpost->nc, &cs, score}};
        if (map_multi_run(e, jobs, a, viterbi != 0, false, nullptr)) {
            std::fill(score, score + ncand, NAN);
            return keep_err();
        }
    }
    if (!cs.why.empty()) set_err("map_post_multi: %s", cs.why.c_str());
    return 0;
}
