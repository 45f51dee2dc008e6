/* sh_eng_map_crf_pack.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * one read of a flip-flop (CRF) model against many candidate base sequences (k_map_crf_pack, sh_map_crf_pack.h).
 * scrappie_hip_map_crf_multi_batch: the network and k_crf<true> of a launch group ONCE (run_staged to STOP_POST), every read's candidates packed
 * end to end into workgroups of one k_map_crf_pack launch on the transitions where k_crf left them in d_E, the candidates too long for a pack
 * through k_map_crf (plan_add + dp_run) on the same transitions, scores back; with a path wanted, a second pass of k_map_crf on each read's best
 * candidate alone while d_E still holds the transitions.  scrappie_hip_map_trans_multi: the same on a host matrix and the process-default engine.
 * The packing itself is host arithmetic in sh_host.c (scrappie_hip_map_crf_pack_plan).  What is here is the family's own: how a candidate becomes
 * cell words, the pack record, the launch, the "no admissible path" rule, the second pass.  Sets, their registry, the layout of a launch and the
 * scatter of its scores, the upload of a host matrix, the batch call and the launch group's stage are sh_eng_post.inc's. */

#define SH_MAP_CRF_PACK_CELLS 1024      /* cells a pack holds unless the debug option "map_crf_pack_cells" says otherwise: the fastest on 16 shared candidates of about 150 bases, and faster than k_map_crf per candidate on a call of ~730 bases and 7 edits of it (profiles/map_crf_multi_rate.txt) */

/* launches of each k_map_crf_pack form in this process: index (vit ? 2 : 0) | (tiled ? 1 : 0) */
static std::atomic<uint64_t> g_map_crf_pack_forms[4];
extern "C" void scrappie_hip_map_crf_pack_form_counts(uint64_t forms[4]) {
    for (int k = 0; k < 4; k++) if (forms) forms[k] = g_map_crf_pack_forms[k].load(std::memory_order_relaxed);
}

/* a PackSet (sh_eng_post.inc) of candidates as k_map_crf_pack reads them */
struct CrfCandSet : PackSet {
    std::vector<size_t> over;                 /* the candidates that take k_map_crf */
    size_t maxL = 0;                          /* the longest candidate that can be mapped */
    size_t maxcell = 0;                       /* cells of its largest pack */
};                                            /* (bytes: a path's second pass apart) */

static size_t map_crf_pack_cells(const scrappie_hip_engine *e) { return e->map_crf_pack_cells < 0 ? (size_t)SH_MAP_CRF_PACK_CELLS : (size_t)e->map_crf_pack_cells; }

/* pack_cells 0: every candidate through k_map_crf */
static void crf_cand_set_build(CrfCandSet &cs, const scrappie_hip_map_target *cand, size_t n, size_t pack_cells) {
    cs.cand = cand; cs.n = n;
    std::vector<size_t> good, len;
    auto bad = [&](size_t k, const std::string &text) { if (cs.why.empty()) cs.why = "candidate " + std::to_string(k) + ": " + text; };
    for (size_t k = 0; k < n; k++) {
        const scrappie_hip_map_target &t = cand[k];
        if (t.poslow || t.poshigh) { bad(k, "bands are not part of this call"); continue; }
        if (!t.seq) { bad(k, "no sequence"); continue; }
        if (t.seqlen == 0) { bad(k, "an empty sequence"); continue; }
        if (t.seqlen > SH_MAP_MAX_SEQ) { bad(k, "a sequence of " + std::to_string(t.seqlen) + " bases is longer than the " + std::to_string(SH_MAP_MAX_SEQ) + " this build maps"); continue; }
        const size_t i = first_non_base(t.seq, t.seqlen);
        if (i < t.seqlen) { bad(k, non_base_text(t.seq, i)); continue; }
        good.push_back(k); len.push_back(t.seqlen);
        cs.maxL = std::max(cs.maxL, t.seqlen);
    }
    std::vector<int> pack(good.size(), -1);
    std::vector<long long> cell(good.size(), -1);
    if (pack_cells && !good.empty()) cs.packs.resize((size_t)scrappie_hip_map_crf_pack_plan(len.data(), good.size(), pack_cells, pack.data(), cell.data()));
    int cur = -1;
    for (size_t j = 0; j < good.size(); j++) {
        const scrappie_hip_map_target &t = cand[good[j]];
        if (pack[j] < 0) { cs.over.push_back(good[j]); cs.bytes += map_crf_read_bytes(t.seqlen, 1, false, false); continue; }
        if (pack[j] != cur) { cur = pack[j]; cs.packs[(size_t)cur] = PackSet::Pack{cs.cellw.size(), 0, cs.packed.size(), 0, 0}; }
        PackSet::Pack &P = cs.packs[(size_t)cur];
        const size_t L = t.seqlen;
        cs.cellw.push_back(SH_MCP_WORD(0, 0, 0, 0, 0));
        for (size_t p = 1; p <= L; p++) cs.cellw.push_back(SH_MCP_WORD(p == L ? P.nitem : 0, p == L, p == 1 ? 1 : 2, t.seq[p - 1], p >= 2 ? t.seq[p - 2] : 0));
        P.ncell += L + 1; P.nitem++;
        cs.packed.push_back(good[j]);
    }
    for (const PackSet::Pack &P : cs.packs) cs.maxcell = std::max(cs.maxcell, P.ncell);
    cs.bytes += cs.cellw.size() * 4 + cs.packs.size() * sizeof(ShMapCrfPack) + n * 4 + 64;
}

/* one read of a launch: where its transitions are (as plan_add takes them), its candidates, and where their scores go ([cs->n], NAN already) */
struct CrfMultiJob { long long trans; int lane; size_t nblock; const CrfCandSet *cs; float *score; };

/* The scores of jobs[] (under mu): every pack of every read as a workgroup of one k_map_crf_pack launch (PackLaunch, sh_eng_post.inc), the candidates
 * left to k_map_crf as one dp_run.  trans: d_E or the uploaded matrices.  A candidate without an admissible path keeps its NAN.  t (may be NULL):
 * t[0] += the kernels, t[1] += copies. */
static int crf_multi_run(scrappie_hip_engine *e, const std::vector<CrfMultiJob> &jobs, const float *trans, bool vit, bool tiled, double *t) {
    hipStream_t s = e->stream;
    std::vector<ShMapCrfPack> pk;
    PackLaunch<CrfCandSet> L;
    L.lay(jobs, [&](size_t j, const PackSet::Pack &P, size_t cell, size_t, size_t out) {
        ShMapCrfPack q{};
        q.trans = jobs[j].trans; q.lane = jobs[j].lane; q.nblock = (int)jobs[j].nblock;
        q.cell = (long long)cell; q.out = (long long)out; q.ncell = (int)P.ncell;
        pk.push_back(q);
    });
    MapCrfPlan over;
    std::vector<std::pair<size_t, size_t>> over_who;          /* (job, candidate) */
    for (size_t j = 0; j < jobs.size(); j++)
        for (size_t k : jobs[j].cs->over) {
            const scrappie_hip_map_target &c = jobs[j].cs->cand[k];
            plan_add(over, jobs[j].trans, jobs[j].lane, jobs[j].nblock, c.seq, c.seqlen, nullptr, nullptr, false);
            over_who.emplace_back(j, k);
        }
    if (!pk.empty()) {
        size_t maxcell = 0;
        for (const auto &kv : L.up) maxcell = std::max(maxcell, kv.first->maxcell);
        const size_t nscore = L.nscore, np = pk.size(), lds = sh_map_crf_pack_lds_bytes(maxcell);
        if (lds > SH_MAP_LDS) return set_err("map_crf_multi: a pack of %zu bytes of LDS", lds);
        if (e->d_mcp_rd.ensure(np * sizeof(ShMapCrfPack)) || e->d_mcp_cell.ensure(L.cellw.size() * 4 + 16) || e->d_mcp_score.ensure(nscore * 4 + 16) ||
            e->h_mcp.ensure(nscore * 4 + 16)) return -1;
        HIPCHK(hipMemcpyAsync(e->d_mcp_rd.p, pk.data(), np * sizeof(ShMapCrfPack), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(e->d_mcp_cell.p, L.cellw.data(), L.cellw.size() * 4, hipMemcpyHostToDevice, s));
        ShMapCrfPackArgs a{};
        a.packs = e->d_mcp_rd.as<ShMapCrfPack>(); a.trans = trans; a.cells = e->d_mcp_cell.as<int>(); a.score = e->d_mcp_score.as<float>();
        Span2 span;
        if (pick_bool([&](auto v, auto tl) {
                using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
                g_map_crf_pack_forms[(v() ? 2 : 0) | (tl() ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
                return launch_k<k_map_crf_pack<v(), LD>>(dim3((unsigned)np), dim3(SH_MAP_NTH), lds, s, a);
            }, vit, tiled)) return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(sh_stream_wait(s));
        span.mark();
        const float *hs = e->h_mcp.as<float>();
        HIPCHK(hipMemcpyAsync(e->h_mcp.p, e->d_mcp_score.p, nscore * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
        L.scatter(jobs, [&](const CrfMultiJob &job, size_t k, size_t slot) {
            if (hs[slot] >= -SH_MAP_BIG / 2) job.score[k] = hs[slot];      /* else no admissible path: NAN stays */
        });
        span.add(t);
    }
    if (!over_who.empty()) {
        std::vector<float> sc(over_who.size(), NAN);
        ShMapCrfArgs a{};
        a.trans = trans;
        if (dp_run(e, over, a, vit, false, tiled, sc.data(), nullptr, t)) return -1;
        for (size_t i = 0; i < over_who.size(); i++) jobs[over_who[i].first].score[over_who[i].second] = sc[i];
    }
    return 0;
}

/* the first candidate of a set that was run and has no admissible path (NAN from the kernels), -1: none */
static long crf_multi_first_unfit(const CrfCandSet &cs, const float *score) {
    long first = -1;
    for (const std::vector<size_t> *v : {&cs.packed, &cs.over})
        for (size_t k : *v)
            if (std::isnan(score[k]) && (first < 0 || (long)k < first)) first = (long)k;
    return first;
}

/* one launch group: reads idx[] of the call (post_group, sh_eng_post.inc), setof[r] the candidates of read r */
static int crf_multi_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const std::vector<const CrfCandSet *> &setof, const std::vector<size_t> &idx,
                           const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_multi_result *out, LaunchCut<MapLoad> &cut) {
    return post_group(e, m, reads, idx, p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
        std::vector<CrfMultiJob> jobs;
        for (const PostRead &q : rd) jobs.push_back(CrfMultiJob{q.boff, q.lane, q.nblock, setof[q.r], out[q.r].score});
        if (crf_multi_run(e, jobs, ro.E, vit, true, e->map_ms + 1)) return -1;
        MapCrfPlan second;                     /* each read's best candidate alone, with its traceback: before anything can overwrite d_E */
        std::vector<size_t> second_who;
        for (size_t j = 0; j < jobs.size(); j++) {
            scrappie_hip_map_multi_result &res = out[rd[j].r];
            res.nblock = jobs[j].nblock;
            res.best = best_finite(res.score, res.ncand);
            const long unfit = crf_multi_first_unfit(*jobs[j].cs, res.score);
            if (unfit >= 0) cut.refuse(rd[j].r, ("candidate " + std::to_string(unfit) + ": " + MAP_CRF_NO_PATH).c_str());
            if (!(vit && want_path) || res.best < 0) continue;
            const scrappie_hip_map_target &t = jobs[j].cs->cand[res.best];
            plan_add(second, jobs[j].trans, jobs[j].lane, jobs[j].nblock, t.seq, t.seqlen, nullptr, nullptr, true);
            second_who.push_back(rd[j].r);
        }
        if (!second_who.empty()) {
            std::vector<float> sc(second_who.size(), NAN);
            std::vector<int32_t *> paths(second_who.size(), nullptr);
            ShMapCrfArgs a{};
            a.trans = ro.E;
            if (dp_run(e, second, a, true, false, true, sc.data(), paths.data(), e->map_ms + 1)) {
                for (int32_t *q : paths) free(q);
                return -1;
            }
            for (size_t k = 0; k < second_who.size(); k++) out[second_who[k]].path = paths[k];
        }
        return 0;
    });
}

extern "C" int scrappie_hip_map_crf_multi_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *cands,
                                                size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_multi_result *out) {
    PostCall c(e, "map_crf_multi_batch");
    if (c.enter(!n || (reads && cands && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_map_multi_result{nullptr, 0, -1, 0, nullptr};
    if (c.open(model, p, [](Model *m) {
            return m->arch != 1 ? set_err("map_crf_multi_batch: model '%s' is a transducer model; its candidates are mapped by scrappie_hip_map_multi_batch", m->name.c_str()) : 0;
        })) return -1;
    Model *m = c.m;
    const bool vit = viterbi != 0, wp = want_path != 0;
    /* the candidates: one set per distinct cand array of the call */
    PackSets<CrfCandSet> sets;
    std::vector<const CrfCandSet *> &setof = sets.of;
    setof.assign(n, nullptr);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = cands[i].ncand;
        out[i].score = (float *)malloc(std::max<size_t>(nc, 1) * sizeof(float));
        if (!out[i].score) { map_multi_blank(out, n); return set_err("map_crf_multi_batch: out of host memory"); }
        std::fill(out[i].score, out[i].score + nc, NAN);
        out[i].ncand = nc;
        if (!nc || !cands[i].cand) continue;
        setof[i] = sets.get(cands[i].cand, nc, [&](CrfCandSet &cs) { crf_cand_set_build(cs, cands[i].cand, nc, map_crf_pack_cells(e)); });
    }
    /* launch groups as scrappie_hip_map_batch cuts them for a flip-flop model; a read adds its tables and scores, the rows of the candidates left to
     * k_map_crf and, with a path, the second pass on its longest candidate */
    LaunchCut<MapLoad> cut{e, "map_crf_multi_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) { return crf_multi_group(e, m, reads, setof, grp, c.p, vit, wp, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (cands[i].ncand && !cands[i].cand) { cut.refuse(i, "no candidates"); continue; }
        const size_t T = c.blocks(cut, i, reads[i]);
        if (T == 0) continue;
        const CrfCandSet *cs = setof[i];
        if (!cs) { out[i].nblock = T; continue; }                  /* no candidates: a read with no scores */
        if (!cs->why.empty()) cut.refuse(i, cs->why.c_str());      /* (its other candidates are scored) */
        if (cs->packed.empty() && cs->over.empty()) { out[i].nblock = T; continue; }
        c.add(cut, i, T, cs->bytes + (vit && wp ? map_crf_read_bytes(cs->maxL, T, false, true) : 0),
              "read and candidates too long for one launch group on this device");
    }
    return c.finish(cut, [&] { map_multi_blank(out, n); });
}

extern "C" int scrappie_hip_map_trans_multi(const_scrappie_matrix tr, const scrappie_hip_map_target *cand, size_t ncand, int viterbi, float *score) {
    const char *const fn = "map_trans_multi";
    if (!tr || (ncand && (!cand || !score))) return set_err("%s: null argument", fn);
    std::fill(score, score + ncand, NAN);
    if (!sh_crf_post_ok(tr)) return set_err("%s: not a transition matrix of 25 rows and at least one block", fn);
    if (tr->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, tr->nc);
    if (ncand == 0) return 0;
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    CrfCandSet cs;
    crf_cand_set_build(cs, cand, ncand, map_crf_pack_cells(e));
    if (!cs.packed.empty() || !cs.over.empty()) {
        const float *dtr = post_upload_trans(e, fn, tr);
        if (!dtr) return -1;
        const std::vector<CrfMultiJob> jobs{CrfMultiJob{0, (int)tr->stride, tr->nc, &cs, score}};
        if (crf_multi_run(e, jobs, dtr, viterbi != 0, false, nullptr)) {
            std::fill(score, score + ncand, NAN);
            return keep_err();
        }
    }
    const long unfit = crf_multi_first_unfit(cs, score);
    if (!cs.why.empty()) set_err("%s: %s", fn, cs.why.c_str());
    else if (unfit >= 0) set_err("%s: candidate %ld: %s", fn, unfit, MAP_CRF_NO_PATH);
    return 0;
}
