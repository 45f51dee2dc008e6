/* sh_eng_crf_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * every single-base edit of a sequence scored against a read of a flip-flop (CRF) model (k_crf_edits_rows, k_crf_edits, sh_crf_edits.h).
 * scrappie_hip_map_crf_edits_batch: the network and k_crf<true> of a launch group once (run_staged to STOP_POST), then per launch of the group's
 * reads -- all of them, or as many as the debug option "crf_edits_budget_kb" lets through -- the forward rows, the backward rows and the combining
 * pass on the transitions where k_crf left them in d_E; results back.  map_crf_edits: the same on a host matrix and the process-default engine.
 * The layout of a launch's row and result buffers is host arithmetic in sh_host.c (scrappie_hip_crf_edits_plan).  What is here is the family's own:
 * the checks a target passes, the records, the three launches, the "no admissible path" rule.  The batch call, the launch group's stage and the
 * upload of a host matrix are sh_eng_post.inc's. */

/* launches of each form in this process: k_crf_edits_rows at (vit ? 4 : 0) | (tiled ? 2 : 0) | (back ? 1 : 0), k_crf_edits at 8 + ((vit ? 2 : 0) | (tiled ? 1 : 0)) */
static std::atomic<uint64_t> g_crf_edits_forms[12];
extern "C" void scrappie_hip_crf_edits_form_counts(uint64_t forms[12]) {
    for (int k = 0; k < 12; k++) if (forms) forms[k] = g_crf_edits_forms[k].load(std::memory_order_relaxed);
}
extern "C" void scrappie_hip_crf_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes) {
    if (!e) return;
    for (int k = 0; k < 3; k++) if (ms) ms[k] = e->crf_edits_ms[k];
    if (launches) *launches = e->crf_edits_launches;
    if (row_bytes) *row_bytes = e->crf_edits_row_bytes;
}

/* why a target cannot be scored; empty: it can */
static std::string crf_edits_target_why(const scrappie_hip_map_target &t) {
    if (t.poslow || t.poshigh) return "bands are not part of this call";
    if (t.seqlen == 0) return "an empty sequence";
    if (!t.seq) return "no sequence";
    const size_t maxL = scrappie_hip_map_crf_lds_max_seq();
    if (t.seqlen > maxL) return "a sequence of " + std::to_string(t.seqlen) + " bases is too long for k_crf_edits (" + std::to_string(maxL) + ": score a window of it)";
    const size_t i = first_non_base(t.seq, t.seqlen);
    if (i < t.seqlen) return non_base_text(t.seq, i);
    return std::string();
}
/* device bytes a read adds to a launch: rows, results, codes, its record and base score */
static size_t crf_edits_read_bytes(size_t L, size_t nblock) {
    return scrappie_hip_crf_edits_row_bytes(L, nblock) + (9 * L + 8) * 4 + L * 4 + sizeof(ShCrfEditsRead) + 64;
}

/* one read of a launch: where its transitions are (as plan_add takes them), its sequence, and where its results go (NAN already; any may be NULL) */
struct CrfEditsJob { long long trans; int lane; size_t nblock; const int *seq; size_t L; float *base, *sub, *del, *ins; };

/* jobs[j0, j1) as one launch of the three kernels (under mu, on the main stream).  trans: d_E or the uploaded matrix. */
static int crf_edits_launch(scrappie_hip_engine *e, const std::vector<CrfEditsJob> &jobs, size_t j0, size_t j1, const float *trans, bool vit, bool tiled) {
    hipStream_t s = e->stream;
    const size_t n = j1 - j0;
    std::vector<size_t> Ls(n), NBs(n);
    std::vector<int> pitch(n), codes;
    std::vector<long long> rows(n), res(n);
    size_t maxL = 0;
    for (size_t k = 0; k < n; k++) { Ls[k] = jobs[j0 + k].L; NBs[k] = jobs[j0 + k].nblock; maxL = std::max(maxL, Ls[k]); }
    long long nres = 0;
    const long long nrow = scrappie_hip_crf_edits_plan(Ls.data(), NBs.data(), n, pitch.data(), rows.data(), res.data(), &nres);
    std::vector<ShCrfEditsRead> rd(n);
    for (size_t k = 0; k < n; k++) {
        const CrfEditsJob &j = jobs[j0 + k];
        ShCrfEditsRead &r = rd[k];
        r.trans = j.trans; r.lane = j.lane; r.nblock = (int)j.nblock; r.seqlen = (int)j.L; r.pitch = pitch[k];
        r.seq = (long long)codes.size(); r.rows = rows[k]; r.res = res[k];
        codes.insert(codes.end(), j.seq, j.seq + j.L);
    }
    const size_t lds = map_crf_lds_bytes(maxL);
    if (lds > SH_MAP_LDS) return set_err("map_crf_edits: rows of %zu bytes of LDS", lds);
    if (e->d_ce_rd.ensure(n * sizeof(ShCrfEditsRead)) || e->d_ce_seq.ensure(codes.size() * 4 + 16) || e->d_ce_rows.ensure((size_t)nrow * 4 + 16) ||
        e->d_ce_res.ensure((size_t)nres * 4 + 16) || e->d_ce_base.ensure(n * 4 + 16) || e->h_ce.ensure(((size_t)nres + n) * 4 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(e->d_ce_rd.p, rd.data(), n * sizeof(ShCrfEditsRead), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_ce_seq.p, codes.data(), codes.size() * 4, hipMemcpyHostToDevice, s));
    ShCrfEditsArgs a{};
    a.rd = e->d_ce_rd.as<ShCrfEditsRead>(); a.trans = trans; a.seq = e->d_ce_seq.as<int>(); a.rows = e->d_ce_rows.as<float>();
    a.res = e->d_ce_res.as<float>(); a.base = e->d_ce_base.as<float>();
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto drop = [&] { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); };
    for (hipEvent_t &x : ev) if (hipEventCreate(&x) != hipSuccess) { drop(); return set_err("map_crf_edits: hipEventCreate failed"); }
    const dim3 chunks((unsigned)n, (unsigned)((maxL + SH_MAP_NTH) / SH_MAP_NTH));
    int rc = 0;
    (void)hipEventRecord(ev[0], s);
    for (int back = 0; back < 2 && !rc; back++) {
        rc = pick_bool([&](auto v, auto tl, auto bk) {
            using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
            g_crf_edits_forms[(v() ? 4 : 0) | (tl() ? 2 : 0) | (bk() ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
            return launch_k<k_crf_edits_rows<v(), LD, bk()>>(dim3((unsigned)n), dim3(SH_MAP_NTH), lds, s, a);
        }, vit, tiled, back != 0);
        (void)hipEventRecord(ev[1 + back], s);
    }
    if (!rc)
        rc = pick_bool([&](auto v, auto tl) {
            using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
            g_crf_edits_forms[8 + ((v() ? 2 : 0) | (tl() ? 1 : 0))].fetch_add(1, std::memory_order_relaxed);
            return launch_k<k_crf_edits<v(), LD>>(chunks, dim3(SH_MAP_NTH), 0, s, a);
        }, vit, tiled);
    (void)hipEventRecord(ev[3], s);
    float *const h = e->h_ce.as<float>();
    if (!rc && (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, e->d_ce_res.p, (size_t)nres * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(h + nres, e->d_ce_base.p, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess || sh_stream_wait(s) != hipSuccess))
        rc = set_err("map_crf_edits: the launch failed");
    if (!rc) {
        for (int k = 0; k < 3; k++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) e->crf_edits_ms[k] += ms;
        }
        e->crf_edits_launches++;
        e->crf_edits_row_bytes += (size_t)nrow * 4;
    }
    drop();
    if (rc) return -1;
    auto put = [](float *dst, const float *src, size_t cnt) {      /* a score below -SH_MAP_BIG / 2: no admissible path, NAN */
        if (!dst) return;
        for (size_t i = 0; i < cnt; i++) dst[i] = src[i] >= -SH_MAP_BIG / 2 ? src[i] : NAN;
    };
    for (size_t k = 0; k < n; k++) {
        const CrfEditsJob &j = jobs[j0 + k];
        const float *r = h + res[k];
        put(j.base, h + nres + k, 1);
        put(j.sub, r, 4 * j.L);
        put(j.ins, r + 4 * j.L, 4 * (j.L + 1));
        if (j.L >= 2) put(j.del, r + 8 * j.L + 4, j.L);           /* (the deletion of an only base leaves no sequence: NAN stays) */
    }
    return 0;
}

/* jobs[] in launches of at most `budget` row and result bytes (0: one launch; a job over the budget goes alone).  t (may be NULL): t[0] += the launches, results included */
static int crf_edits_run(scrappie_hip_engine *e, const std::vector<CrfEditsJob> &jobs, const float *trans, bool vit, bool tiled, size_t budget, double *t) {
    Span2 span;
    size_t j0 = 0, bytes = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        const size_t b = crf_edits_read_bytes(jobs[j].L, jobs[j].nblock);
        if (budget && j > j0 && bytes + b > budget) {
            if (crf_edits_launch(e, jobs, j0, j, trans, vit, tiled)) return -1;
            j0 = j; bytes = 0;
        }
        bytes += b;
    }
    if (j0 < jobs.size() && crf_edits_launch(e, jobs, j0, jobs.size(), trans, vit, tiled)) return -1;
    span.mark();
    span.add(t);
    return 0;
}

/* ------------------------------------------------------------------ */
/* per-read symbol                                                      */
/* ------------------------------------------------------------------ */
extern "C" int map_crf_edits(const_scrappie_matrix tr, const int *seq, size_t seqlen, int viterbi, float *base, float *sub, float *del, float *ins) {
    const char *const fn = "map_crf_edits";
    if (base) *base = NAN;
    if (seq || seqlen == 0) {                                /* (without a sequence the lengths of the arrays are not known to be its) */
        if (sub) std::fill(sub, sub + 4 * seqlen, NAN);
        if (del) std::fill(del, del + seqlen, NAN);
        if (ins) std::fill(ins, ins + 4 * (seqlen + 1), NAN);
    }
    if (!tr || (!seq && seqlen)) return set_err("%s: null argument", fn);
    if (!sh_crf_post_ok(tr)) return set_err("%s: not a transition matrix of 25 rows and at least one block", fn);
    if (tr->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, tr->nc);
    const std::string why = crf_edits_target_why(scrappie_hip_map_target{seq, seqlen, nullptr, nullptr});
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }      /* every score NAN, the reason as the error text */
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    const float *dtr = post_upload_trans(e, fn, tr);
    if (!dtr) return -1;
    const std::vector<CrfEditsJob> jobs{CrfEditsJob{0, (int)tr->stride, tr->nc, seq, seqlen, base, sub, del, ins}};
    if (crf_edits_run(e, jobs, dtr, viterbi != 0, false, 0, nullptr)) return keep_err();
    return 0;
}

/* ------------------------------------------------------------------ */
/* batched                                                              */
/* ------------------------------------------------------------------ */
static void edits_blank(scrappie_hip_edits_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].sub); free(r[i].del); free(r[i].ins); r[i] = scrappie_hip_edits_result{NAN, nullptr, nullptr, nullptr, 0, 0}; }
}
extern "C" void scrappie_hip_free_edits_results(scrappie_hip_edits_result *r, size_t n) { if (r) edits_blank(r, n); }

extern "C" int scrappie_hip_map_crf_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                                const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    PostCall c(e, "map_crf_edits_batch");
    if (c.enter(!n || (reads && targets && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_edits_result{NAN, nullptr, nullptr, nullptr, 0, 0};
    if (c.open(model, p, [](Model *m) {
            return m->arch != 1 ? set_err("map_crf_edits_batch: model '%s' is a transducer model; edits are scored for reads of flip-flop (CRF) models only", m->name.c_str()) : 0;
        })) return -1;
    Model *m = c.m;
    const bool vit = viterbi != 0;
    for (double &x : e->crf_edits_ms) x = 0.0;
    e->crf_edits_launches = 0; e->crf_edits_row_bytes = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t L = targets[i].seq ? targets[i].seqlen : 0;
        out[i].sub = (float *)malloc(std::max<size_t>(4 * L, 1) * sizeof(float));
        out[i].del = (float *)malloc(std::max<size_t>(L, 1) * sizeof(float));
        out[i].ins = (float *)malloc(4 * (L + 1) * sizeof(float));
        if (!out[i].sub || !out[i].del || !out[i].ins) { edits_blank(out, n); return set_err("map_crf_edits_batch: out of host memory"); }
        std::fill(out[i].sub, out[i].sub + 4 * L, NAN);
        std::fill(out[i].del, out[i].del + L, NAN);
        std::fill(out[i].ins, out[i].ins + 4 * (L + 1), NAN);
        out[i].seqlen = L;
    }
    /* launch groups as scrappie_hip_map_batch cuts them for a flip-flop model; a read adds its three row matrices and its results */
    LaunchCut<MapLoad> cut{e, "map_crf_edits_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) {
        return post_group(e, m, reads, grp, c.p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
            std::vector<CrfEditsJob> jobs;
            for (const PostRead &q : rd) {
                scrappie_hip_edits_result &r = out[q.r];
                r.nblock = q.nblock;
                jobs.push_back(CrfEditsJob{q.boff, q.lane, q.nblock, targets[q.r].seq, targets[q.r].seqlen, &r.base, r.sub, r.del, r.ins});
            }
            return crf_edits_run(e, jobs, ro.E, vit, true, e->dbg_crf_edits_budget, e->map_ms + 1);
        });
    };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        const std::string why = crf_edits_target_why(targets[i]);
        if (!why.empty()) { cut.refuse(i, why.c_str()); continue; }
        const size_t T = c.blocks(cut, i, reads[i]);
        if (T == 0) continue;
        c.add(cut, i, T, crf_edits_read_bytes(targets[i].seqlen, T), "read and sequence too long for one launch group on this device");
    }
    return c.finish(cut, [&] { edits_blank(out, n); });
}
