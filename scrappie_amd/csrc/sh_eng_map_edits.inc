/* sh_eng_map_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * every single-base edit of a sequence scored against a read of a transducer model (k_map_edits_rows, k_map_edits, sh_map_edits.h).
 * scrappie_hip_map_edits_batch: the network and S1 of a launch group once (run_staged to STOP_POST), then per launch of the group's reads -- all of
 * them, or as many as the debug option "map_edits_budget_kb" lets through -- the forward rows, the backward rows and the combining pass on the
 * posterior where S1 left it in d_E; results back.  map_post_edits: the same on a host posterior and the process-default engine.
 * The layout of a launch's row and result buffers is host arithmetic in sh_host.c (scrappie_hip_map_edits_plan).  What is here is the family's own:
 * the checks a target passes, the k-mer states of its bases, the records, the three launches, the "no admissible path" rule.  The batch call, the
 * launch group's stage and the upload of a host matrix are sh_eng_post.inc's; the result type and its release are sh_eng_crf_edits.inc's. */

/* launches of each form in this process: k_map_edits_rows at (vit ? 4 : 0) | (tiled ? 2 : 0) | (back ? 1 : 0), k_map_edits at 8 + ((vit ? 2 : 0) | (tiled ? 1 : 0)) */
static std::atomic<uint64_t> g_map_edits_forms[12];
extern "C" void scrappie_hip_map_edits_form_counts(uint64_t forms[12]) {
    for (int k = 0; k < 12; k++) if (forms) forms[k] = g_map_edits_forms[k].load(std::memory_order_relaxed);
}
extern "C" void scrappie_hip_map_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes) {
    if (!e) return;
    for (int k = 0; k < 3; k++) if (ms) ms[k] = e->map_edits_ms[k];
    if (launches) *launches = e->map_edits_launches;
    if (row_bytes) *row_bytes = e->map_edits_row_bytes;
}

/* k of a posterior of nr = 4^k + 1 rows, 1 .. SH_ME_K; 0: none */
static int map_edits_kmer(size_t nr) {
    size_t states = 4;
    for (int k = 1; k <= SH_ME_K; k++, states *= 4)
        if (nr == states + 1) return k;
    return 0;
}
/* dynamic LDS of k_map_edits: two buffers of SH_ME_CH columns */
static size_t map_edits_col_lds(size_t nr) { return 2 * (size_t)SH_ME_CH * ((nr + 3) & ~(size_t)3) * 4; }

/* why a target cannot be scored; empty: it can */
static std::string map_edits_target_why(const scrappie_hip_map_target &t, int k) {
    if (t.poslow || t.poshigh) return "bands are not part of this call";
    if (t.seqlen == 0) return "an empty sequence";
    if (!t.seq) return "no sequence";
    if (t.seqlen < (size_t)k) return "a sequence of " + std::to_string(t.seqlen) + " bases is shorter than the model's k-mer (" + std::to_string(k) + ")";
    const size_t maxL = scrappie_hip_map_edits_max_bases((size_t)k);
    if (t.seqlen > maxL) return "a sequence of " + std::to_string(t.seqlen) + " bases is too long for k_map_edits (" + std::to_string(maxL) + ": score a window of it)";
    const size_t i = first_non_base(t.seq, t.seqlen);
    if (i < t.seqlen) return non_base_text(t.seq, i);
    return std::string();
}
/* device bytes a read adds to a launch: rows, results, state and base codes, its record and base score */
static size_t map_edits_read_bytes(size_t L, size_t k, size_t nblock) {
    return scrappie_hip_map_edits_row_bytes(L, k, nblock) + (9 * L + 8) * 4 + 2 * L * 4 + sizeof(ShMapEditsRead) + 64;
}

/* one read of a launch: where its posterior is (as plan_add takes it), its bases, and where its results go (NAN already; any may be NULL) */
struct MapEditsJob { long long post; int lane; size_t nblock; const int *seq; size_t L; float *base, *sub, *del, *ins; };

/* jobs[j0, j1) as one launch of the three kernels (under mu, on the main stream).  a: the posterior, its shape, k and the penalties. */
static int map_edits_launch(scrappie_hip_engine *e, const std::vector<MapEditsJob> &jobs, size_t j0, size_t j1, ShMapEditsArgs a, bool vit, bool tiled) {
    hipStream_t s = e->stream;
    const size_t n = j1 - j0, K = (size_t)a.k;
    std::vector<size_t> Ls(n), NBs(n);
    std::vector<int> pitch(n), codes;
    std::vector<long long> rows(n), res(n);
    size_t maxL = 0;
    for (size_t k = 0; k < n; k++) { Ls[k] = jobs[j0 + k].L; NBs[k] = jobs[j0 + k].nblock; maxL = std::max(maxL, Ls[k]); }
    long long nres = 0;
    const long long nrow = scrappie_hip_map_edits_plan(Ls.data(), NBs.data(), n, K, pitch.data(), rows.data(), res.data(), &nres);
    if (nrow < 0) return set_err("map_edits: a sequence shorter than the k-mer reached the launch");
    std::vector<ShMapEditsRead> rd(n);
    for (size_t k = 0; k < n; k++) {
        const MapEditsJob &j = jobs[j0 + k];
        ShMapEditsRead &r = rd[k];
        r.post = j.post; r.lane = j.lane; r.nblock = (int)j.nblock; r.nbase = (int)j.L; r.pitch = pitch[k];
        r.rows = rows[k]; r.res = res[k];
        r.seq = (long long)codes.size();
        unsigned code = 0;                                   /* the k-mer states, the oldest base the most significant (encode_bases_to_integers) */
        const unsigned mask = K >= 16 ? ~0u : (1u << (2 * K)) - 1u;
        for (size_t i = 0; i < j.L; i++) {
            code = ((code << 2) | (unsigned)j.seq[i]) & mask;
            if (i + 1 >= K) codes.push_back((int)code);
        }
        r.bases = (long long)codes.size();
        codes.insert(codes.end(), j.seq, j.seq + j.L);
    }
    const size_t lds_rows = map_lds_bytes(maxL - K + 1), lds_cols = map_edits_col_lds((size_t)a.nr);
    if (lds_rows > SH_MAP_LDS || lds_cols > SH_MAP_LDS) return set_err("map_edits: %zu and %zu bytes of LDS", lds_rows, lds_cols);
    if (e->d_me_rd.ensure(n * sizeof(ShMapEditsRead)) || e->d_me_seq.ensure(codes.size() * 4 + 16) || e->d_me_rows.ensure((size_t)nrow * 4 + 16) ||
        e->d_me_res.ensure((size_t)nres * 4 + 16) || e->d_me_base.ensure(n * 4 + 16) || e->h_me.ensure(((size_t)nres + n) * 4 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(e->d_me_rd.p, rd.data(), n * sizeof(ShMapEditsRead), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_me_seq.p, codes.data(), codes.size() * 4, hipMemcpyHostToDevice, s));
    a.rd = e->d_me_rd.as<ShMapEditsRead>(); a.seq = e->d_me_seq.as<int>(); a.rows = e->d_me_rows.as<float>();
    a.res = e->d_me_res.as<float>(); a.base = e->d_me_base.as<float>();
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto drop = [&] { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); };
    for (hipEvent_t &x : ev) if (hipEventCreate(&x) != hipSuccess) { drop(); return set_err("map_edits: hipEventCreate failed"); }
    const dim3 chunks((unsigned)n, (unsigned)((maxL + SH_MAP_NTH) / SH_MAP_NTH));
    int rc = 0;
    (void)hipEventRecord(ev[0], s);
    for (int back = 0; back < 2 && !rc; back++) {
        rc = pick_bool([&](auto v, auto tl, auto bk) {
            g_map_edits_forms[(v() ? 4 : 0) | (tl() ? 2 : 0) | (bk() ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
            return launch_k<k_map_edits_rows<v(), tl(), bk()>>(dim3((unsigned)n), dim3(SH_MAP_NTH), lds_rows, s, a);
        }, vit, tiled, back != 0);
        (void)hipEventRecord(ev[1 + back], s);
    }
    if (!rc)
        rc = pick_bool([&](auto v, auto tl) {
            g_map_edits_forms[8 + ((v() ? 2 : 0) | (tl() ? 1 : 0))].fetch_add(1, std::memory_order_relaxed);
            return launch_k<k_map_edits<v(), tl()>>(chunks, dim3(SH_MAP_NTH), lds_cols, s, a);
        }, vit, tiled);
    (void)hipEventRecord(ev[3], s);
    float *const h = e->h_me.as<float>();
    if (!rc && (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, e->d_me_res.p, (size_t)nres * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(h + nres, e->d_me_base.p, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess || sh_stream_wait(s) != hipSuccess))
        rc = set_err("map_edits: the launch failed");
    if (!rc) {
        for (int k = 0; k < 3; k++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) e->map_edits_ms[k] += ms;
        }
        e->map_edits_launches++;
        e->map_edits_row_bytes += (size_t)nrow * 4;
    }
    drop();
    if (rc) return -1;
    auto put = [](float *dst, const float *src, size_t cnt) {      /* a score below -SH_MAP_BIG / 2: no admissible path, NAN */
        if (!dst) return;
        for (size_t i = 0; i < cnt; i++) dst[i] = src[i] >= -SH_MAP_BIG / 2 ? src[i] : NAN;
    };
    for (size_t k = 0; k < n; k++) {
        const MapEditsJob &j = jobs[j0 + k];
        const float *r = h + res[k];
        if (j.base) *j.base = h[nres + k];                         /* k_map's score as it is */
        put(j.sub, r, 4 * j.L);
        put(j.ins, r + 4 * j.L, 4 * (j.L + 1));
        if (j.L > K) put(j.del, r + 8 * j.L + 4, j.L);            /* (a deletion from k bases leaves no state: NAN stays) */
    }
    return 0;
}

/* jobs[] in launches of at most `budget` row and result bytes (0: one launch; a job over the budget goes alone).  t (may be NULL): t[0] += the launches, results included */
static int map_edits_run(scrappie_hip_engine *e, const std::vector<MapEditsJob> &jobs, const ShMapEditsArgs &a, bool vit, bool tiled, size_t budget, double *t) {
    Span2 span;
    size_t j0 = 0, bytes = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        const size_t b = map_edits_read_bytes(jobs[j].L, (size_t)a.k, jobs[j].nblock);
        if (budget && j > j0 && bytes + b > budget) {
            if (map_edits_launch(e, jobs, j0, j, a, vit, tiled)) return -1;
            j0 = j; bytes = 0;
        }
        bytes += b;
    }
    if (j0 < jobs.size() && map_edits_launch(e, jobs, j0, jobs.size(), a, vit, tiled)) return -1;
    span.mark();
    span.add(t);
    return 0;
}

/* ------------------------------------------------------------------ */
/* per-read symbol                                                      */
/* ------------------------------------------------------------------ */
extern "C" int map_post_edits(const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, int viterbi, float *base,
                              float *sub, float *del, float *ins) {
    const char *const fn = "map_post_edits";
    if (base) *base = NAN;
    if (seq || seqlen == 0) {                                /* (without a sequence the lengths of the arrays are not known to be its) */
        if (sub) std::fill(sub, sub + 4 * seqlen, NAN);
        if (del) std::fill(del, del + seqlen, NAN);
        if (ins) std::fill(ins, ins + 4 * (seqlen + 1), NAN);
    }
    if (!lp || (!seq && seqlen)) return set_err("%s: null argument", fn);
    const int k = map_edits_kmer(lp->nr);
    if (!k) return set_err("%s: a posterior of %zu rows is not 4^k + 1 states for k = 1 .. %d", fn, lp->nr, SH_ME_K);
    if (lp->nc == 0) return set_err("%s: a posterior of no blocks", fn);
    if (lp->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, lp->nc);
    if (lp->stride % 4 != 0 || lp->stride < ((lp->nr + 3) & ~(size_t)3))
        return set_err("%s: a posterior whose columns are %zu floats apart (whole 16-byte pieces of %zu states)", fn, lp->stride, lp->nr);
    const std::string why = map_edits_target_why(scrappie_hip_map_target{seq, seqlen, nullptr, nullptr}, k);
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }      /* every score NAN, the reason as the error text */
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    ShMapEditsArgs a{};
    a.post = post_upload_dense(e, fn, lp);
    if (!a.post) return -1;
    a.pstride = (long long)lp->stride; a.nr = (int)lp->nr; a.k = k;
    a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
    const std::vector<MapEditsJob> jobs{MapEditsJob{0, 0, lp->nc, seq, seqlen, base, sub, del, ins}};
    if (map_edits_run(e, jobs, a, viterbi != 0, false, 0, nullptr)) return keep_err();
    return 0;
}

/* ------------------------------------------------------------------ */
/* batched                                                              */
/* ------------------------------------------------------------------ */
extern "C" int scrappie_hip_map_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                            const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    PostCall c(e, "map_edits_batch");
    if (c.enter(!n || (reads && targets && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_edits_result{NAN, nullptr, nullptr, nullptr, 0, 0};
    int K = 0;
    if (c.open(model, p, [&](Model *m) {
            if (m->arch == 1)
                return set_err("map_edits_batch: model '%s' is a flip-flop (CRF) model; its edits are scored with scrappie_hip_map_crf_edits_batch", m->name.c_str());
            K = map_edits_kmer((size_t)m->NS);
            if (!K) return set_err("map_edits_batch: model '%s' has %d states, not 4^k + 1 for k = 1 .. %d", m->name.c_str(), m->NS, SH_ME_K);
            return ((m->NS + 3) / 4 - 1) / 4 < m->ff_mtiles ? 0 : set_err("map_edits_batch: model '%s' has %d states in %d chunks of 16", m->name.c_str(), m->NS, m->ff_mtiles);
        })) return -1;
    Model *m = c.m;
    const bool vit = viterbi != 0;
    for (double &x : e->map_edits_ms) x = 0.0;
    e->map_edits_launches = 0; e->map_edits_row_bytes = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t L = targets[i].seq ? targets[i].seqlen : 0;
        out[i].sub = (float *)malloc(std::max<size_t>(4 * L, 1) * sizeof(float));
        out[i].del = (float *)malloc(std::max<size_t>(L, 1) * sizeof(float));
        out[i].ins = (float *)malloc(4 * (L + 1) * sizeof(float));
        if (!out[i].sub || !out[i].del || !out[i].ins) { edits_blank(out, n); return set_err("map_edits_batch: out of host memory"); }
        std::fill(out[i].sub, out[i].sub + 4 * L, NAN);
        std::fill(out[i].del, out[i].del + L, NAN);
        std::fill(out[i].ins, out[i].ins + 4 * (L + 1), NAN);
        out[i].seqlen = L;
    }
    /* launch groups as scrappie_hip_map_batch cuts them for a transducer model; a read adds its two row matrices and its results */
    LaunchCut<MapLoad> cut{e, "map_edits_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) {
        return post_group(e, m, reads, grp, c.p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
            std::vector<MapEditsJob> jobs;
            for (const PostRead &q : rd) {
                scrappie_hip_edits_result &r = out[q.r];
                r.nblock = q.nblock;
                jobs.push_back(MapEditsJob{q.boff, q.lane, q.nblock, targets[q.r].seq, targets[q.r].seqlen, &r.base, r.sub, r.del, r.ins});
            }
            ShMapEditsArgs a{};
            a.E = ro.E; a.sums = ro.sums; a.nr = m->NS; a.nchunk = m->ff_mtiles; a.k = K; a.min_prob = c.p->min_prob;
            a.stay_pen = c.p->stay_pen; a.skip_pen = c.p->skip_pen; a.local_pen = c.p->local_pen;
            return map_edits_run(e, jobs, a, vit, true, e->dbg_map_edits_budget, e->map_ms + 1);
        });
    };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        const std::string why = map_edits_target_why(targets[i], K);
        if (!why.empty()) { cut.refuse(i, why.c_str()); continue; }
        const size_t T = c.blocks(cut, i, reads[i]);
        if (T == 0) continue;
        c.add(cut, i, T, map_edits_read_bytes(targets[i].seqlen, (size_t)K, T), "read and sequence too long for one launch group on this device");
    }
    return c.finish(cut, [&] { edits_blank(out, n); });
}
