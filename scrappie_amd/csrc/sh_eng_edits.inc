/* sh_eng_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * the host side that the two engines which score EVERY single-base edit of a sequence share (k_crf_edits_rows / k_crf_edits and k_map_edits_rows /
 * k_map_edits: sh_eng_crf_edits.inc, sh_eng_map_edits.inc).  edits_launch: reads of a launch group, or one host matrix, through the forward rows, the
 * backward rows and the combining pass, laid out by the family's planner in sh_host.c, results back with the "no admissible path" rule; edits_run:
 * the jobs of a call cut by a byte budget; edits_nan / edits_one: the head and the tail of a per-read symbol on the process-default engine;
 * edits_batch: the batch call -- the network of a launch group once (post_group, sh_eng_post.inc), then edits_run on what it left in d_E; the result
 * type's release; form counts and timing.  A family says what is its own in an EditsTraits. */

/* What a family says of its record Rec: Args, its kernels' arguments; name, as its error texts begin; state(e), the EditsState of the engine it uses;
 * plan(jobs, L, nblock, n, a, pitch, rows, res, res_floats), its planner of the ABI on the n jobs' lengths and block counts (below 0: refused);
 * read_bytes(j, a), the device bytes job j adds to a launch: rows, results, codes, its record and base score; fill(r, j, codes, a): the record's own fields and what the read appends to
 * codes; lds_rows(maxL, a) and lds_edits(a), the dynamic LDS of the two kernels, and lds_err(rows, edits), its text where either is too much;
 * launch_rows / launch_edits: launch_k on its kernels' forms; base_as_is: the base score goes out as the kernel wrote it (else through the "no
 * admissible path" rule); del_from(a): the fewest bases a deletion leaves something of; target_why(t, a): why a target cannot be scored, empty: it
 * can; read_why(t, nblock, a): the same once the read's block count is known; model_ok(m) and args(m, p, ro): the batch call's check of the model and
 * its kernels' arguments on what the network left; run(e, jobs, a, vit, tiled, budget, t): the jobs of a launch group through edits_run. */
template <class Rec> struct EditsTraits;

/* launches of each form in this process: the rows kernel at (vit ? 4 : 0) | (tiled ? 2 : 0) | (back ? 1 : 0), the combining one at 8 + ((vit ? 2 : 0) | (tiled ? 1 : 0)) */
template <class Rec> static std::atomic<uint64_t> g_edits_forms[12];
template <class Rec>
static void edits_form_counts(uint64_t forms[12]) {
    for (int k = 0; k < 12; k++) if (forms) forms[k] = g_edits_forms<Rec>[k].load(std::memory_order_relaxed);
}
static void edits_timing(const EditsState &d, double ms[3], size_t *launches, size_t *row_bytes) {
    for (int k = 0; k < 3; k++) if (ms) ms[k] = d.ms[k];
    if (launches) *launches = d.launches;
    if (row_bytes) *row_bytes = d.row_bytes;
}

/* one read of a launch: where its posterior or transitions are (as plan_add takes them), its sequence, and where its results go (NAN already; any may be NULL) */
struct EditsJob { long long at; int lane; size_t nblock; const int *seq; size_t L; float *base, *sub, *del, *ins; const size_t *lo, *hi; /* its band, or NULL */ };

/* jobs[j0, j1) as one launch of the three kernels (under mu, on the main stream).  a: what the kernels take of the caller. */
template <class Rec>
static int edits_launch(scrappie_hip_engine *e, const std::vector<EditsJob> &jobs, size_t j0, size_t j1, typename EditsTraits<Rec>::Args a, bool vit, bool tiled) {
    using T = EditsTraits<Rec>;
    hipStream_t s = e->stream;
    EditsState &d = T::state(e);
    const size_t n = j1 - j0;
    std::vector<size_t> Ls(n), NBs(n);
    std::vector<int> pitch(n), codes;
    std::vector<long long> rows(n), res(n);
    size_t maxL = 0;
    for (size_t k = 0; k < n; k++) { Ls[k] = jobs[j0 + k].L; NBs[k] = jobs[j0 + k].nblock; maxL = std::max(maxL, Ls[k]); }
    long long nres = 0;
    const long long nrow = T::plan(jobs.data() + j0, Ls.data(), NBs.data(), n, a, pitch.data(), rows.data(), res.data(), &nres);
    if (nrow < 0) return set_err("%s: a sequence shorter than the k-mer reached the launch", T::name);
    std::vector<Rec> rd(n);
    for (size_t k = 0; k < n; k++) {
        const EditsJob &j = jobs[j0 + k];
        Rec &r = rd[k];
        r.lane = j.lane; r.nblock = (int)j.nblock; r.pitch = pitch[k]; r.rows = rows[k]; r.res = res[k];
        T::fill(r, j, codes, a);
    }
    const size_t lds_rows = T::lds_rows(maxL, a), lds_edits = T::lds_edits(a);
    if (lds_rows > SH_MAP_LDS || lds_edits > SH_MAP_LDS) return T::lds_err(lds_rows, lds_edits);
    if (d.rd.ensure(n * sizeof(Rec)) || d.seq.ensure(codes.size() * 4 + 16) || d.rows.ensure((size_t)nrow * 4 + 16) || d.res.ensure((size_t)nres * 4 + 16) ||
        d.base.ensure(n * 4 + 16) || d.h.ensure(((size_t)nres + n) * 4 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(d.rd.p, rd.data(), n * sizeof(Rec), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.seq.p, codes.data(), codes.size() * 4, hipMemcpyHostToDevice, s));
    a.rd = d.rd.as<Rec>(); a.seq = d.seq.as<int>(); a.rows = d.rows.as<float>(); a.res = d.res.as<float>(); a.base = d.base.as<float>();
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto drop = [&] { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); };
    for (hipEvent_t &x : ev) if (hipEventCreate(&x) != hipSuccess) { drop(); return set_err("%s: hipEventCreate failed", T::name); }
    const dim3 chunks((unsigned)n, (unsigned)((maxL + SH_MAP_NTH) / SH_MAP_NTH));
    int rc = 0;
    (void)hipEventRecord(ev[0], s);
    for (int back = 0; back < 2 && !rc; back++) {
        g_edits_forms<Rec>[(vit ? 4 : 0) | (tiled ? 2 : 0) | back].fetch_add(1, std::memory_order_relaxed);
        rc = T::launch_rows(dim3((unsigned)n), lds_rows, s, a, vit, tiled, back != 0);
        (void)hipEventRecord(ev[1 + back], s);
    }
    if (!rc) {
        g_edits_forms<Rec>[8 + ((vit ? 2 : 0) | (tiled ? 1 : 0))].fetch_add(1, std::memory_order_relaxed);
        rc = T::launch_edits(chunks, lds_edits, s, a, vit, tiled);
    }
    (void)hipEventRecord(ev[3], s);
    float *const h = d.h.as<float>();
    if (!rc && (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, d.res.p, (size_t)nres * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(h + nres, d.base.p, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess || sh_stream_wait(s) != hipSuccess))
        rc = set_err("%s: the launch failed", T::name);
    if (!rc) {
        for (int k = 0; k < 3; k++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) d.ms[k] += ms;
        }
        d.launches++;
        d.row_bytes += (size_t)nrow * 4;
    }
    drop();
    if (rc) return -1;
    auto put = [](float *dst, const float *src, size_t cnt) {      /* a score below -SH_MAP_BIG / 2: no admissible path, NAN */
        if (!dst) return;
        for (size_t i = 0; i < cnt; i++) dst[i] = src[i] >= -SH_MAP_BIG / 2 ? src[i] : NAN;
    };
    for (size_t k = 0; k < n; k++) {
        const EditsJob &j = jobs[j0 + k];
        const float *r = h + res[k];
        if (!T::base_as_is) put(j.base, h + nres + k, 1);
        else if (j.base) *j.base = h[nres + k];
        put(j.sub, r, 4 * j.L);
        put(j.ins, r + 4 * j.L, 4 * (j.L + 1));
        if (j.L >= T::del_from(a)) put(j.del, r + 8 * j.L + 4, j.L);      /* (a deletion that leaves nothing to map to: NAN stays) */
    }
    return 0;
}

/* jobs[] in launches of at most `budget` row and result bytes (0: one launch; a job over the budget goes alone).  t (may be NULL): t[0] += the launches, results included */
template <class Rec>
static int edits_run(scrappie_hip_engine *e, const std::vector<EditsJob> &jobs, const typename EditsTraits<Rec>::Args &a, bool vit, bool tiled, size_t budget, double *t) {
    Span2 span;
    size_t j0 = 0, bytes = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        const size_t b = EditsTraits<Rec>::read_bytes(jobs[j], a);
        if (budget && j > j0 && bytes + b > budget) {
            if (edits_launch<Rec>(e, jobs, j0, j, a, vit, tiled)) return -1;
            j0 = j; bytes = 0;
        }
        bytes += b;
    }
    if (j0 < jobs.size() && edits_launch<Rec>(e, jobs, j0, jobs.size(), a, vit, tiled)) return -1;
    span.mark();
    span.add(t);
    return 0;
}

/* ------------------------------------------------------------------ */
/* per-read symbols                                                     */
/* ------------------------------------------------------------------ */
/* the head of a per-read symbol: every score NAN before any check */
static void edits_nan(const int *seq, size_t seqlen, float *base, float *sub, float *del, float *ins) {
    if (base) *base = NAN;
    if (!seq && seqlen) return;                              /* (without a sequence the lengths of the arrays are not known to be its) */
    if (sub) std::fill(sub, sub + 4 * seqlen, NAN);
    if (del) std::fill(del, del + seqlen, NAN);
    if (ins) std::fill(ins, ins + 4 * (seqlen + 1), NAN);
}
/* its tail, after the family's checks: the one read of job on the process-default engine.  upload(e, a), under mu: the host matrix onto the device
 * and into a; 0 or -1. */
template <class Rec, class Upload>
static int edits_one(const EditsJob &job, typename EditsTraits<Rec>::Args a, bool vit, Upload &&upload) {
    scrappie_hip_engine *e = default_engine();
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    if (upload(e, a)) return -1;
    if (edits_run<Rec>(e, std::vector<EditsJob>{job}, a, vit, false, 0, nullptr)) return keep_err();
    return 0;
}

/* ------------------------------------------------------------------ */
/* batched                                                              */
/* ------------------------------------------------------------------ */
static void edits_blank(scrappie_hip_edits_result *r, size_t n) {
    for (size_t i = 0; i < n; i++) { free(r[i].sub); free(r[i].del); free(r[i].ins); r[i] = scrappie_hip_edits_result{NAN, nullptr, nullptr, nullptr, 0, 0}; }
}
extern "C" void scrappie_hip_free_edits_results(scrappie_hip_edits_result *r, size_t n) { if (r) edits_blank(r, n); }

/* The batch call of a family, fn as its error texts begin: launch groups as scrappie_hip_map_batch cuts them for the family's models; a read adds
 * its row matrices and its results.  Each launch group: reads idx[] of the call through post_group, then edits_run under the family's budget. */
template <class Rec>
static int edits_batch(const char *fn, scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                       const scrappie_hip_params *p, bool vit, scrappie_hip_edits_result *out) {
    using T = EditsTraits<Rec>;
    PostCall c(e, fn);
    if (c.enter(!n || (reads && targets && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_edits_result{NAN, nullptr, nullptr, nullptr, 0, 0};
    if (c.open(model, p, T::model_ok)) return -1;
    Model *m = c.m;
    EditsState &d = T::state(e);
    for (double &x : d.ms) x = 0.0;
    d.launches = 0; d.row_bytes = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t L = targets[i].seq ? targets[i].seqlen : 0;
        out[i].sub = (float *)malloc(std::max<size_t>(4 * L, 1) * sizeof(float));
        out[i].del = (float *)malloc(std::max<size_t>(L, 1) * sizeof(float));
        out[i].ins = (float *)malloc(4 * (L + 1) * sizeof(float));
        if (!out[i].sub || !out[i].del || !out[i].ins) { edits_blank(out, n); return set_err("%s: out of host memory", fn); }
        std::fill(out[i].sub, out[i].sub + 4 * L, NAN);
        std::fill(out[i].del, out[i].del + L, NAN);
        std::fill(out[i].ins, out[i].ins + 4 * (L + 1), NAN);
        out[i].seqlen = L;
    }
    LaunchCut<MapLoad> cut{e, fn};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) {
        return post_group(e, m, reads, grp, c.p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
            std::vector<EditsJob> jobs;
            for (const PostRead &q : rd) {
                scrappie_hip_edits_result &r = out[q.r];
                r.nblock = q.nblock;
                jobs.push_back(EditsJob{q.boff, q.lane, q.nblock, targets[q.r].seq, targets[q.r].seqlen, &r.base, r.sub, r.del, r.ins, targets[q.r].poslow, targets[q.r].poshigh});
            }
            return T::run(e, jobs, T::args(m, c.p, ro), vit, true, d.budget, e->map_ms + 1);
        });
    };
    const typename T::Args a = T::args(m, c.p, RunOut());   /* (what the checks and the byte count read of it does not depend on the launch group) */
    for (size_t i = 0; i < n && !cut.failed; i++) {
        const std::string why = T::target_why(targets[i], a);
        if (!why.empty()) { cut.refuse(i, why.c_str()); continue; }
        const size_t nb = c.blocks(cut, i, reads[i]);
        if (nb == 0) continue;
        const std::string why_nb = T::read_why(targets[i], nb, a);
        if (!why_nb.empty()) { cut.refuse(i, why_nb.c_str()); continue; }
        const EditsJob j{0, 0, nb, targets[i].seq, targets[i].seqlen, nullptr, nullptr, nullptr, nullptr, targets[i].poslow, targets[i].poshigh};
        c.add(cut, i, nb, T::read_bytes(j, a), "read and sequence too long for one launch group on this device");
    }
    return c.finish(cut, [&] { edits_blank(out, n); });
}
