/* sh_eng_crf_find.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * short sequences (motifs) searched INSIDE reads of a flip-flop (CRF) model (k_crf_find, sh_crf_find.h).  find_crf_sequences_viterbi
 * on the process-default engine (the caller's host matrix uploaded, the reference-layout loader) and scrappie_hip_find_batch: the
 * network and k_crf<true> of a launch group (run_staged to STOP_POST), every pack of every read of the group in ONE k_crf_find
 * launch on the transitions where k_crf left them in d_E, under the engine's lock; scores, positions and call scores back.  The
 * packing itself is host arithmetic in sh_host.c (scrappie_hip_crf_find_plan).  What is here is the family's own: how a motif becomes cell
 * words, the pack record, the launch, positions and call scores, the "fits nowhere" rule.  Sets, their registry, the layout of a launch and
 * the scatter of its scores, the upload of a host matrix, the batch call and the launch group's stage are sh_eng_post.inc's. */

#define SH_CRF_FIND_CELLS 512       /* cells a pack holds unless the debug option "crf_find_cells" says otherwise: two chunks of 256 threads; the fastest on 24 motifs of 40 bases with positions and on 96 of 24 (profiles/crf_find_rate.txt), 256 within 3 % of it */

/* launches of each k_crf_find form in this process: index (pos ? 2 : 0) | (tiled ? 1 : 0) */
static std::atomic<uint64_t> g_crf_find_forms[4];
extern "C" void scrappie_hip_crf_find_form_counts(uint64_t forms[4]) {
    for (int k = 0; k < 4; k++) if (forms) forms[k] = g_crf_find_forms[k].load(std::memory_order_relaxed);
}

static const char *const CRF_FIND_NO_FIT = "no occurrence fits the read (the motif has more bases than the read has entries)";

/* a PackSet (sh_eng_post.inc) of motifs as k_crf_find reads them; its packs are never empty: a set without a motif to search is one pack of the
 * five U cells (the call score) */
struct FindSet : PackSet {
    size_t maxcell = 0;                       /* cells of its largest pack */
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
        const size_t i = first_non_base(t.seq, t.seqlen);
        if (i < t.seqlen) { bad(k, non_base_text(t.seq, i)); continue; }
        good.push_back(k); len.push_back(t.seqlen);
    }
    std::vector<int> pack(good.size(), -1);               /* (none stays -1: the planner's bound is the one checked above) */
    std::vector<long long> cell(good.size(), -1);
    const size_t np = good.empty() ? 0 : (size_t)scrappie_hip_crf_find_plan(len.data(), good.size(), pack_cells, pack.data(), cell.data());
    cs.packs.resize(std::max<size_t>(np, 1));
    auto open = [&](size_t p) {
        cs.packs[p] = PackSet::Pack{cs.cellw.size(), 0, cs.packed.size(), 5, 0};
        for (int s = 0; s < 5; s++) cs.cellw.push_back(SH_CFD_WORD(0, SH_CFD_U, s, 0, 0));
    };
    if (np == 0) open(0);
    int cur = -1;
    for (size_t j = 0; j < good.size(); j++) {
        const scrappie_hip_map_target &t = cand[good[j]];
        if (pack[j] != cur) { cur = pack[j]; open((size_t)cur); }
        PackSet::Pack &P = cs.packs[(size_t)cur];
        const size_t L = t.seqlen;
        for (size_t p = 1; p < L; p++) cs.cellw.push_back(SH_CFD_WORD(0, p == 1 ? SH_CFD_B1 : SH_CFD_INT, 0, t.seq[p - 1], p >= 2 ? t.seq[p - 2] : 0));
        for (int s = 0; s < 5; s++) cs.cellw.push_back(SH_CFD_WORD(P.nitem, L >= 2 ? SH_CFD_V : SH_CFD_V1, s, t.seq[L - 1], L >= 2 ? t.seq[L - 2] : 0));
        P.ncell += L + 4; P.nitem++;
        cs.packed.push_back(good[j]);
    }
    for (const PackSet::Pack &P : cs.packs) cs.maxcell = std::max(cs.maxcell, P.ncell);
    cs.bytes = cs.cellw.size() * 4 + cs.packs.size() * (sizeof(ShCrfFindPack) + 4) + cs.packed.size() * 12 + 64;
}

/* one read of a launch: where its transitions are (as plan_add takes them), its motifs, and where the results go ([cs->n] each, NAN / -1 already;
 * begin and end may be NULL) */
struct FindJob { long long trans; int lane; size_t nblock; const FindSet *cs; float *score; int32_t *begin, *end; float call; };

/* The results of jobs[] (under mu): every pack of every read as a workgroup of one k_crf_find launch (PackLaunch, sh_eng_post.inc).  trans: d_E or
 * the uploaded matrices.  t (may be NULL): t[0] += the kernel, t[1] += copies. */
static int find_run(scrappie_hip_engine *e, std::vector<FindJob> &jobs, const float *trans, bool tiled, bool pos, double *t) {
    if (jobs.empty()) return 0;
    hipStream_t s = e->stream;
    std::vector<ShCrfFindPack> pk;
    std::vector<size_t> pack0(jobs.size(), 0);           /* a job's first pack: where its call score comes back */
    PackLaunch<FindSet> L;
    L.lay(jobs, [&](size_t j, const PackSet::Pack &P, size_t cell, size_t, size_t out) {
        if (&P == &jobs[j].cs->packs[0]) pack0[j] = pk.size();
        ShCrfFindPack q{};
        q.trans = jobs[j].trans; q.lane = jobs[j].lane; q.nblock = (int)jobs[j].nblock;
        q.cell = (long long)cell; q.out = (long long)out; q.ncell = (int)P.ncell;
        pk.push_back(q);
    });
    size_t maxcell = 0;
    for (const auto &kv : L.up) maxcell = std::max(maxcell, kv.first->maxcell);
    const std::vector<int> &cellw = L.cellw;
    const size_t nscore = L.nscore, np = pk.size(), lds = sh_crf_find_lds_bytes(maxcell, pos);
    if (lds > SH_MAP_LDS) return set_err("crf_find: a pack of %zu bytes of LDS", lds);
    if (e->d_cfd_rd.ensure(np * sizeof(ShCrfFindPack)) || e->d_cfd_cell.ensure(cellw.size() * 4 + 16) || e->d_cfd_score.ensure(nscore * 4 + 16) ||
        e->d_cfd_pos.ensure(nscore * 8 + 16) || e->d_cfd_call.ensure(np * 4 + 16) || e->h_cfd.ensure(nscore * 12 + np * 4 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(e->d_cfd_rd.p, pk.data(), np * sizeof(ShCrfFindPack), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_cfd_cell.p, cellw.data(), cellw.size() * 4, hipMemcpyHostToDevice, s));
    ShCrfFindArgs a{};
    a.packs = e->d_cfd_rd.as<ShCrfFindPack>(); a.trans = trans; a.cells = e->d_cfd_cell.as<int>();
    a.score = e->d_cfd_score.as<float>(); a.pos = e->d_cfd_pos.as<int2>(); a.call = e->d_cfd_call.as<float>();
    Span2 span;
    if (pick_bool([&](auto ps, auto tl) {
            using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
            g_crf_find_forms[(ps() ? 2 : 0) | (tl() ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
            return launch_k<k_crf_find<ps(), LD>>(dim3((unsigned)np), dim3(SH_MAP_NTH), lds, s, a);
        }, pos, tiled)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    span.mark();
    const float *hc = e->h_cfd.as<float>(), *hs = hc + np;
    const int2 *hp = (const int2 *)(hs + nscore + ((np + nscore) & 1));      /* 8-byte aligned */
    HIPCHK(hipMemcpyAsync((void *)hc, e->d_cfd_call.p, np * 4, hipMemcpyDeviceToHost, s));
    if (nscore) HIPCHK(hipMemcpyAsync((void *)hs, e->d_cfd_score.p, nscore * 4, hipMemcpyDeviceToHost, s));
    if (nscore && pos) HIPCHK(hipMemcpyAsync((void *)hp, e->d_cfd_pos.p, nscore * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    for (size_t j = 0; j < jobs.size(); j++) jobs[j].call = hc[pack0[j]];
    L.scatter(jobs, [&](FindJob &job, size_t k, size_t slot) {
        const float sc = hs[slot];
        if (!(sc >= -SH_MAP_BIG / 2)) return;             /* no occurrence fits: NAN and -1 stay */
        job.score[k] = sc;
        if (pos && job.begin) job.begin[k] = hp[slot].x;
        if (pos && job.end) job.end[k] = hp[slot].y;
    });
    span.add(t);
    return 0;
}

/* the first motif of a set that was searched and fits nowhere (NAN from the kernel's score), -1: none */
static long find_first_unfit(const FindSet &cs, const float *score) {
    long first = -1;
    for (size_t k : cs.packed)
        if (std::isnan(score[k]) && (first < 0 || (long)k < first)) first = (long)k;
    return first;
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
    const float *dtr = post_upload_trans(e, fn, tr);
    if (!dtr) return -1;
    std::vector<FindJob> jobs{FindJob{0, (int)tr->stride, tr->nc, &cs, score, begin, end, NAN}};
    if (find_run(e, jobs, dtr, false, begin || end, nullptr)) {
        std::fill(score, score + nmotif, NAN);
        return keep_err();
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

/* one launch group: reads idx[] of the call (post_group, sh_eng_post.inc), setof[r] the motifs of read r */
static int find_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const std::vector<const FindSet *> &setof, const std::vector<size_t> &idx,
                      const scrappie_hip_params *p, bool pos, scrappie_hip_find_result *out, LaunchCut<MapLoad> &cut) {
    return post_group(e, m, reads, idx, p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
        std::vector<FindJob> jobs;
        for (const PostRead &q : rd) jobs.push_back(FindJob{q.boff, q.lane, q.nblock, setof[q.r], out[q.r].score, out[q.r].begin, out[q.r].end, NAN});
        if (find_run(e, jobs, ro.E, true, pos, e->map_ms + 1)) return -1;
        for (size_t j = 0; j < jobs.size(); j++) {
            scrappie_hip_find_result &res = out[rd[j].r];
            res.nblock = jobs[j].nblock;
            res.call_score = jobs[j].call;
            res.best = best_finite(res.score, res.nmotif);
            const long unfit = find_first_unfit(*jobs[j].cs, res.score);
            if (unfit >= 0) cut.refuse(rd[j].r, ("motif " + std::to_string(unfit) + ": " + CRF_FIND_NO_FIT).c_str());
        }
        return 0;
    });
}

extern "C" int scrappie_hip_find_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *motifs, size_t n,
                                       const scrappie_hip_params *p, int want_pos, scrappie_hip_find_result *out) {
    PostCall c(e, "find_batch");
    if (c.enter(!n || (reads && motifs && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_find_result{nullptr, nullptr, nullptr, 0, NAN, -1, 0};
    if (c.open(model, p, [](Model *m) {
            return m->arch != 1 ? set_err("find_batch: model '%s' is a transducer model; sequences are searched inside reads of flip-flop (CRF) models only", m->name.c_str()) : 0;
        })) return -1;
    Model *m = c.m;
    const bool pos = want_pos != 0;
    /* the motifs: one set per distinct cand array of the call */
    PackSets<FindSet> sets;
    std::vector<const FindSet *> &setof = sets.of;
    setof.assign(n, nullptr);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = motifs[i].cand ? motifs[i].ncand : 0;
        out[i].score = (float *)malloc(std::max<size_t>(nc, 1) * sizeof(float));
        if (pos) { out[i].begin = (int32_t *)malloc(std::max<size_t>(nc, 1) * 4); out[i].end = (int32_t *)malloc(std::max<size_t>(nc, 1) * 4); }
        if (!out[i].score || (pos && (!out[i].begin || !out[i].end))) { find_blank(out, n); return set_err("find_batch: out of host memory"); }
        std::fill(out[i].score, out[i].score + nc, NAN);
        if (pos) { std::fill(out[i].begin, out[i].begin + nc, -1); std::fill(out[i].end, out[i].end + nc, -1); }
        out[i].nmotif = nc;
        setof[i] = sets.get(nc ? motifs[i].cand : nullptr, nc, [&](FindSet &cs) { find_set_build(cs, motifs[i].cand, nc, crf_find_cells(e)); });
    }
    /* launch groups as scrappie_hip_map_batch cuts them; a read adds its cell words, packs and results */
    LaunchCut<MapLoad> cut{e, "find_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) { return find_group(e, m, reads, setof, grp, c.p, pos, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        if (motifs[i].ncand && !motifs[i].cand) cut.refuse(i, "no motifs");
        const size_t T = c.blocks(cut, i, reads[i]);
        if (T == 0) continue;
        const FindSet *cs = setof[i];
        if (!cs->why.empty()) cut.refuse(i, cs->why.c_str());      /* (its other motifs are searched) */
        c.add(cut, i, T, cs->bytes, "read and motifs too long for one launch group on this device");
    }
    return c.finish(cut, [&] { find_blank(out, n); });
}
