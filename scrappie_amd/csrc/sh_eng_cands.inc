/* sh_eng_cands.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * the host side that the two engines which score one read against many candidate sequences packed into workgroups share (k_map_pack and
 * k_map_crf_pack: sh_eng_map_pack.inc, sh_eng_map_crf_pack.inc).  cand_set_build: a cand array checked, packed by the family's planner in sh_host.c
 * and laid out as its kernel reads it; cand_run: every pack of every read of a launch as a workgroup of one launch (PackLaunch, sh_eng_post.inc),
 * the candidates too long for a pack through the family's per-candidate kernel (plan_add + dp_run) on the same posterior or transitions, scores
 * back; cand_group / cand_batch: the batch call -- the network of a launch group once (post_group), cand_run on what it left in d_E, the best
 * candidate and, with a path wanted, a second pass of the per-candidate kernel on it alone while d_E still holds it; cand_one: the tail of a
 * per-read symbol on the process-default engine; the result type's release; form counts.  A family says what is its own in a CandTraits. */

/* What a family says of its pack record Pack: Rec, the record of its per-candidate kernel (DpTraits, sh_eng_post.inc); name, as the texts of a
 * launch begin; no_path: a score below -SH_MAP_BIG / 2 stays NAN and is reported as "no admissible path"; default_cells, the cells a pack holds
 * unless the engine's PackState says otherwise; state(e), the PackState of the engine it uses; plan, its planner of the ABI; why(fn, t, nr, nblock):
 * why a candidate with a sequence and no bands cannot be run, empty: it can; add(cs, P, t): t's cell words (and first cells) behind the set's and
 * its cells onto P.ncell; lds(P), the dynamic LDS of a pack; read_bytes(L, nblock, path), the device bytes of a candidate through the
 * per-candidate kernel; fill(q, job, P, first): the record's own fields; launch(grid, lds, s, a, st, vit, tiled): launch_k on its kernel's forms;
 * model_ok(m) and args(m, p, ro): the batch call's check of the model and the per-candidate kernel's arguments on what the network left. */
template <class Pack> struct CandTraits;

/* launches of each pack kernel form in this process: index (vit ? 2 : 0) | (tiled ? 1 : 0) */
template <class Pack> static std::atomic<uint64_t> g_cand_forms[4];
template <class Pack>
static void cand_form_counts(uint64_t forms[4]) {
    for (int k = 0; k < 4; k++) if (forms) forms[k] = g_cand_forms<Pack>[k].load(std::memory_order_relaxed);
}

/* a PackSet (sh_eng_post.inc) of candidates as the family's pack kernel reads them */
struct CandSet : PackSet {
    std::vector<size_t> over;                 /* the candidates that take the per-candidate kernel */
    size_t maxL = 0;                          /* the longest candidate that can be mapped */
    size_t lds = 0;                           /* dynamic LDS of its largest pack */
};                                            /* (bytes: a path's second pass apart) */

template <class Pack>
static size_t cand_cells(scrappie_hip_engine *e) {
    const int c = CandTraits<Pack>::state(e).cells;
    return c < 0 ? CandTraits<Pack>::default_cells : (size_t)c;
}

/* nr: posterior rows; nblock: of the read where it is known (else 1: the caller checks its reads); pack_cells 0: every candidate through the
 * per-candidate kernel */
template <class Pack>
static void cand_set_build(CandSet &cs, const char *fn, const scrappie_hip_map_target *cand, size_t n, size_t nr, size_t nblock, size_t pack_cells) {
    using T = CandTraits<Pack>;
    cs.cand = cand; cs.n = n;
    std::vector<size_t> good, len;
    for (size_t k = 0; k < n; k++) {
        const scrappie_hip_map_target &t = cand[k];
        const std::string text = t.poslow || t.poshigh ? "bands are not part of this call" : !t.seq ? "no sequence" : T::why(fn, t, nr, nblock);
        if (!text.empty()) {
            if (cs.why.empty()) cs.why = "candidate " + std::to_string(k) + ": " + text;
            continue;
        }
        good.push_back(k); len.push_back(t.seqlen);
        cs.maxL = std::max(cs.maxL, t.seqlen);
    }
    std::vector<int> pack(good.size(), -1);
    std::vector<long long> cell(good.size(), -1);
    if (pack_cells && !good.empty()) cs.packs.resize((size_t)T::plan(len.data(), good.size(), pack_cells, pack.data(), cell.data()));
    int cur = -1;
    for (size_t j = 0; j < good.size(); j++) {
        const scrappie_hip_map_target &t = cand[good[j]];
        if (pack[j] < 0) { cs.over.push_back(good[j]); cs.bytes += T::read_bytes(t.seqlen, 1, false); continue; }
        if (pack[j] != cur) { cur = pack[j]; cs.packs[(size_t)cur] = PackSet::Pack{cs.cellw.size(), cs.firsts.size(), cs.packed.size(), 0, 0}; }
        T::add(cs, cs.packs[(size_t)cur], t);
        cs.packs[(size_t)cur].nitem++;
        cs.packed.push_back(good[j]);
    }
    for (const PackSet::Pack &P : cs.packs) cs.lds = std::max(cs.lds, T::lds(P));
    cs.bytes += (cs.cellw.size() + cs.firsts.size() + n) * 4 + cs.packs.size() * sizeof(Pack) + 64;
}

/* one read of a launch: where its posterior or transitions are (as plan_add takes them), its candidates, and where their scores go ([cs->n], NAN already) */
struct CandJob { long long at; int lane; size_t nblock; const CandSet *cs; float *score; };

/* The scores of jobs[] (under mu): every pack of every read as a workgroup of one launch of the family's pack kernel, the candidates left to its
 * per-candidate kernel as one dp_run.  a: the posterior or the transitions and what else the kernels take of the caller.  Where the family says
 * no_path, a candidate without an admissible path keeps its NAN.  t (may be NULL): t[0] += the kernels, t[1] += copies. */
template <class Pack>
static int cand_run(scrappie_hip_engine *e, const std::vector<CandJob> &jobs, const typename DpTraits<typename CandTraits<Pack>::Rec>::Args &a, bool vit,
                    bool tiled, double *t) {
    using T = CandTraits<Pack>;
    hipStream_t s = e->stream;
    PackState &d = T::state(e);
    std::vector<Pack> pk;
    PackLaunch<CandSet> L;
    L.lay(jobs, [&](size_t j, const PackSet::Pack &P, size_t cell, size_t first, size_t out) {
        Pack q{};
        q.lane = jobs[j].lane; q.nblock = (int)jobs[j].nblock; q.cell = (long long)cell; q.out = (long long)out; q.ncell = (int)P.ncell;
        T::fill(q, jobs[j], P, first);
        pk.push_back(q);
    });
    DpPlan<typename T::Rec> over;
    std::vector<std::pair<size_t, size_t>> over_who;          /* (job, candidate) */
    for (size_t j = 0; j < jobs.size(); j++)
        for (size_t k : jobs[j].cs->over) {
            const scrappie_hip_map_target &c = jobs[j].cs->cand[k];
            plan_add(over, jobs[j].at, jobs[j].lane, jobs[j].nblock, c.seq, c.seqlen, nullptr, nullptr, false);
            over_who.emplace_back(j, k);
        }
    if (!pk.empty()) {
        size_t lds = 0;
        for (const auto &kv : L.up) lds = std::max(lds, kv.first->lds);
        const size_t nscore = L.nscore, np = pk.size();
        if (lds > SH_MAP_LDS) return set_err("%s: a pack of %zu bytes of LDS", T::name, lds);
        if (d.rd.ensure(np * sizeof(Pack)) || d.cell.ensure(L.cellw.size() * 4 + 16) || (!L.firsts.empty() && d.first.ensure(L.firsts.size() * 4 + 16)) ||
            d.score.ensure(nscore * 4 + 16) || d.h.ensure(nscore * 4 + 16)) return -1;
        HIPCHK(hipMemcpyAsync(d.rd.p, pk.data(), np * sizeof(Pack), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.cell.p, L.cellw.data(), L.cellw.size() * 4, hipMemcpyHostToDevice, s));
        if (!L.firsts.empty()) HIPCHK(hipMemcpyAsync(d.first.p, L.firsts.data(), L.firsts.size() * 4, hipMemcpyHostToDevice, s));
        Span2 span;
        g_cand_forms<Pack>[(vit ? 2 : 0) | (tiled ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
        if (T::launch(dim3((unsigned)np), lds, s, a, d, vit, tiled)) return -1;
        HIPCHK(hipGetLastError());
        HIPCHK(sh_stream_wait(s));
        span.mark();
        const float *hs = d.h.as<float>();
        HIPCHK(hipMemcpyAsync(d.h.p, d.score.p, nscore * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
        L.scatter(jobs, [&](const CandJob &job, size_t k, size_t slot) {
            if (!T::no_path || hs[slot] >= -SH_MAP_BIG / 2) job.score[k] = hs[slot];      /* else no admissible path: NAN stays */
        });
        span.add(t);
    }
    if (!over_who.empty()) {
        std::vector<float> sc(over_who.size(), NAN);
        if (dp_run(e, over, a, vit, false, tiled, sc.data(), nullptr, t)) return -1;
        for (size_t i = 0; i < over_who.size(); i++) jobs[over_who[i].first].score[over_who[i].second] = sc[i];
    }
    return 0;
}

/* the first candidate of a set that was run and has no admissible path (NAN from the kernels), -1: none */
static long cand_first_unfit(const CandSet &cs, const float *score) {
    long first = -1;
    for (const std::vector<size_t> *v : {&cs.packed, &cs.over})
        for (size_t k : *v)
            if (std::isnan(score[k]) && (first < 0 || (long)k < first)) first = (long)k;
    return first;
}

/* ------------------------------------------------------------------ */
/* per-read symbols                                                     */
/* ------------------------------------------------------------------ */
/* The tail of a per-read symbol, after its own checks (score[] NAN already): the one read of nblock blocks on the process-default engine.
 * upload(e, a), under mu: the host matrix onto the device and into a; 0 or -1.  Every candidate that can be run is scored; the first that cannot
 * (or, where the family says no_path, has none) is the error text of a call that returns 0. */
template <class Pack, class Upload>
static int cand_one(const char *fn, const scrappie_hip_map_target *cand, size_t ncand, size_t nr, size_t nblock, int lane, bool vit, float *score,
                    typename DpTraits<typename CandTraits<Pack>::Rec>::Args a, Upload &&upload) {
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    CandSet cs;
    cand_set_build<Pack>(cs, fn, cand, ncand, nr, nblock, cand_cells<Pack>(e));
    if (!cs.packed.empty() || !cs.over.empty()) {
        if (upload(e, a)) return -1;
        if (cand_run<Pack>(e, std::vector<CandJob>{CandJob{0, lane, nblock, &cs, score}}, a, vit, false, nullptr)) {
            std::fill(score, score + ncand, NAN);
            return keep_err();
        }
    }
    const long unfit = CandTraits<Pack>::no_path ? cand_first_unfit(cs, score) : -1;
    if (!cs.why.empty()) set_err("%s: %s", fn, cs.why.c_str());
    else if (unfit >= 0) set_err("%s: candidate %ld: %s", fn, unfit, MAP_CRF_NO_PATH);
    return 0;
}

/* ------------------------------------------------------------------ */
/* batched                                                              */
/* ------------------------------------------------------------------ */
static void map_multi_blank(scrappie_hip_map_multi_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].score); free(r[i].path); r[i] = scrappie_hip_map_multi_result{nullptr, 0, -1, 0, nullptr}; }
}
extern "C" void scrappie_hip_free_map_multi_results(scrappie_hip_map_multi_result *r, size_t n) { if (r) map_multi_blank(r, n); }

/* one launch group: reads idx[] of the call (post_group, sh_eng_post.inc), setof[r] the candidates of read r */
template <class Pack>
static int cand_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const std::vector<const CandSet *> &setof, const std::vector<size_t> &idx,
                      const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_multi_result *out, LaunchCut<MapLoad> &cut) {
    using T = CandTraits<Pack>;
    return post_group(e, m, reads, idx, p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
        std::vector<CandJob> jobs;
        for (const PostRead &q : rd) jobs.push_back(CandJob{q.boff, q.lane, q.nblock, setof[q.r], out[q.r].score});
        const auto a = T::args(m, p, ro);
        if (cand_run<Pack>(e, jobs, a, vit, true, e->map_ms + 1)) return -1;
        DpPlan<typename T::Rec> second;        /* each read's best candidate alone, with its traceback: before anything can overwrite d_E */
        std::vector<size_t> second_who;
        for (size_t j = 0; j < jobs.size(); j++) {
            scrappie_hip_map_multi_result &res = out[rd[j].r];
            res.nblock = jobs[j].nblock;
            res.best = best_finite(res.score, res.ncand);
            const long unfit = T::no_path ? cand_first_unfit(*jobs[j].cs, res.score) : -1;
            if (unfit >= 0) cut.refuse(rd[j].r, ("candidate " + std::to_string(unfit) + ": " + MAP_CRF_NO_PATH).c_str());
            if (!(vit && want_path) || res.best < 0) continue;
            const scrappie_hip_map_target &t = jobs[j].cs->cand[res.best];
            plan_add(second, jobs[j].at, jobs[j].lane, jobs[j].nblock, t.seq, t.seqlen, nullptr, nullptr, true);
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

/* The batch call of a family, fn as its error texts begin: one set per distinct cand array of the call; launch groups as scrappie_hip_map_batch
 * cuts them for the family's models; a read adds its tables and scores, the rows of the candidates left to the per-candidate kernel and, with a
 * path, the second pass on its longest candidate. */
template <class Pack>
static int cand_batch(const char *fn, scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *cands, size_t n,
                      const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_multi_result *out) {
    using T = CandTraits<Pack>;
    PostCall c(e, fn);
    if (c.enter(!n || (reads && cands && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_map_multi_result{nullptr, 0, -1, 0, nullptr};
    if (c.open(model, p, T::model_ok)) return -1;
    Model *m = c.m;
    PackSets<CandSet> sets;
    std::vector<const CandSet *> &setof = sets.of;
    setof.assign(n, nullptr);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = cands[i].ncand;
        out[i].score = (float *)malloc(std::max<size_t>(nc, 1) * sizeof(float));
        if (!out[i].score) { map_multi_blank(out, n); return set_err("%s: out of host memory", fn); }
        std::fill(out[i].score, out[i].score + nc, NAN);
        out[i].ncand = nc;
        if (!nc || !cands[i].cand) continue;
        setof[i] = sets.get(cands[i].cand, nc, [&](CandSet &cs) { cand_set_build<Pack>(cs, fn, cands[i].cand, nc, (size_t)m->NS, 1, cand_cells<Pack>(e)); });
    }
    LaunchCut<MapLoad> cut{e, fn};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) { return cand_group<Pack>(e, m, reads, setof, grp, c.p, vit, want_path, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (cands[i].ncand && !cands[i].cand) { cut.refuse(i, "no candidates"); continue; }
        const size_t nb = c.blocks(cut, i, reads[i]);
        if (nb == 0) continue;
        const CandSet *cs = setof[i];
        if (!cs) { out[i].nblock = nb; continue; }                 /* no candidates: a read with no scores */
        if (!cs->why.empty()) cut.refuse(i, cs->why.c_str());      /* (its other candidates are scored) */
        if (cs->packed.empty() && cs->over.empty()) { out[i].nblock = nb; continue; }
        c.add(cut, i, nb, cs->bytes + (vit && want_path ? T::read_bytes(cs->maxL, nb, true) : 0),
              "read and candidates too long for one launch group on this device");
    }
    return c.finish(cut, [&] { map_multi_blank(out, n); });
}
