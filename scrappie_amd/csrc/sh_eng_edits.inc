/* sh_eng_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * the host side that the two engines which score EVERY single-base edit of a sequence share (k_crf_edits_rows / k_crf_edits and k_map_edits_rows /
 * k_map_edits: sh_eng_crf_edits.inc, sh_eng_map_edits.inc).  edits_launch: reads of a launch group, or one host matrix, through the forward rows, the
 * backward rows and the combining pass, laid out by the family's planner in sh_host.c, results back with the "no admissible path" rule; edits_run:
 * the jobs of a call cut by a byte budget; EditsForm: a family's traits without and with a band, from what the family says once; edits_nan /
 * edits_one / edits_one_of: the head and the tail of a per-read symbol on the process-default engine; edits_batch: the batch call -- the network of
 * a launch group once (post_group, sh_eng_post.inc), then edits_run on what it left in d_E; the result type's release; form counts, the banded
 * forms' scratch and timing. */

/* What the driver asks of a record Rec -- EditsTraits<Rec>, which a family file names as an EditsForm<F, BAND> (below): Args, its kernels' arguments;
 * name, as its error texts begin; state(e), the EditsState of the engine it uses; plan(jobs, L, nblock, n, a, pitch, rows, res, res_floats), its
 * planner of the ABI on the n jobs' lengths and block counts (below 0: refused); read_bytes(j, a), the device bytes job j adds to a launch: rows,
 * results, codes, its record and base score; fill(r, j, codes, a): the record's own fields and what the read appends to codes; lds_rows(maxL, a) and
 * lds_edits(a), the dynamic LDS of the two kernels, and lds_err(rows, edits), its text where either is too much; launch_rows / launch_edits: launch_k
 * on its kernels' forms; base_as_is: the base score goes out as the kernel wrote it (else through the "no admissible path" rule); del_from(a): the
 * fewest bases a deletion leaves something of; target_why(t, a): why a target cannot be scored, empty: it can; read_why(t, nblock, a): the same once
 * the read's block count is known; model_ok(fn, m) and args(m, p, ro): the batch call's check of the model and its kernels' arguments on what the
 * network left; run(e, jobs, a, vit, tiled, budget, t): the jobs of a launch group through edits_run. */
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
/* a family's two forms                                                 */
/* ------------------------------------------------------------------ */
/* A family F says once, for both forms: Rec<BAND> and Args<BAND>; name[BAND]; base_as_is, state(e), del_from(a); lds_rows, lds_edits and
 * lds_err(name, rows, edits); plan<BAND>(L, nblock, lo, hi, n, a, ...), its unbanded planner or its band planner; row_bytes(j, a) and
 * code_ints, the row bytes of a job without a band and the int32 per base it puts into codes; fill(r, j, codes, a); seq_why(t, a), what a sequence
 * must be; model_ok(fn, band, m), args(m, p, ro) of the unbanded form and as<BAND>(a), another form's arguments as this one's; band_entries(nblock),
 * band_row_bytes(lo, hi, nblock) and band_why(t, nblock, a), why a band does not fit the read (empty: it does); rows<BAND>(f, vit, tiled, back) and
 * edits<BAND>(f, vit, tiled, width): f(kernel_c<the form>()); widths, the positions per workgroup its banded combining kernel is built for;
 * set_width(a, e, vit), width_of(a) and count_width(width, vit, tiled): the one a banded launch takes, and its counter.  All else of a form
 * follows here. */
template <auto K> using kernel_c = std::integral_constant<decltype(K), K>;
/* what a family whose banded combining kernel has the one width, SH_MAP_NTH, inherits */
struct EditsOneWidth {
    static constexpr int widths[1] = {SH_MAP_NTH};
    template <class A> static void set_width(A &, const scrappie_hip_engine *, bool) {}
    template <class A> static int width_of(const A &) { return SH_MAP_NTH; }
    static void count_width(int, bool, bool) {}
};

template <class F, bool BAND> struct EditsForm {
    using Rec = typename F::template Rec<BAND>;
    using Args = typename F::template Args<BAND>;
    using U = EditsForm<F, false>;
    static constexpr const char *name = F::name[BAND];
    static constexpr bool base_as_is = F::base_as_is;
    static EditsState &state(scrappie_hip_engine *e) { return F::state(e); }
    static size_t del_from(const Args &a) { return F::del_from(a); }
    static long long plan(const EditsJob *jobs, const size_t *L, const size_t *nblock, size_t n, const Args &a, int *pitch, long long *rows, long long *res, long long *res_floats) {
        std::vector<const size_t *> lo(BAND ? n : 0), hi(BAND ? n : 0);
        for (size_t k = 0; k < lo.size(); k++) { lo[k] = jobs[k].lo; hi[k] = jobs[k].hi; }
        return F::template plan<BAND>(L, nblock, lo.data(), hi.data(), n, a, pitch, rows, res, res_floats);
    }
    /* (a job without a band in a banded call: what it costs the unbanded launch it goes to) */
    static size_t read_bytes(const EditsJob &j, const Args &a) {
        const bool band = BAND && j.lo && j.hi;
        const size_t own = band ? F::band_row_bytes(j.lo, j.hi, j.nblock) + 2 * F::band_entries(j.nblock) * 4 + sizeof(Rec) : F::row_bytes(j, a) + sizeof(typename U::Rec);
        return own + (9 * j.L + 8) * 4 + F::code_ints * j.L * 4 + 64;
    }
    /* in a band the record carries the band's offset and the band travels as int32 behind the read's codes */
    static void fill(Rec &r, const EditsJob &j, std::vector<int> &codes, const Args &a) {
        F::fill(r, j, codes, a);
        if constexpr (BAND) {
            r.band = (long long)codes.size();
            for (const size_t *b : {j.lo, j.hi})
                for (size_t t = 0; t < F::band_entries(j.nblock); t++) codes.push_back((int)b[t]);
        }
    }
    static size_t lds_rows(size_t maxL, const Args &a) { return F::lds_rows(maxL, a); }
    static size_t lds_edits(const Args &a) { return F::lds_edits(a); }
    static int lds_err(size_t rows, size_t edits) { return F::lds_err(name, rows, edits); }
    static int launch_rows(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled, bool back) {
        return F::template rows<BAND>([&](auto k) { return launch_k<decltype(k)::value>(grid, dim3(SH_MAP_NTH), lds, s, a); }, vit, tiled, back);
    }
    /* (grid.y: chunks of SH_MAP_NTH positions; at a smaller width as many times more, and a workgroup past the sequence returns) */
    static int launch_edits(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled) {
        const int w = F::width_of(a);
        F::count_width(w, vit, tiled);
        return F::template edits<BAND>([&](auto k) { return launch_k<decltype(k)::value>(dim3(grid.x, grid.y * (SH_MAP_NTH / w)), dim3(w), lds, s, a); }, vit, tiled, w);
    }
    static std::string target_why(const scrappie_hip_map_target &t, const Args &a) {
        if (BAND ? !t.poslow != !t.poshigh : t.poslow || t.poshigh) return BAND ? "a band needs both poslow and poshigh" : "bands are not part of this call";
        return F::seq_why(t, a);
    }
    static std::string read_why(const scrappie_hip_map_target &t, size_t nblock, const Args &a) { return BAND && t.poslow ? F::band_why(t, nblock, a) : std::string(); }
    static int model_ok(const char *fn, Model *m) { return F::model_ok(fn, BAND, m); }
    static Args args(const Model *m, const scrappie_hip_params *p, const RunOut &ro) { return F::template as<BAND>(F::args(m, p, ro)); }
    /* the jobs with a band through the banded forms at the engine's width, those without through the unbanded ones, each under the budget */
    static int run(scrappie_hip_engine *e, const std::vector<EditsJob> &jobs, const Args &a, bool vit, bool tiled, size_t budget, double *t) {
        if constexpr (!BAND) return edits_run<Rec>(e, jobs, a, vit, tiled, budget, t);
        else {
            std::vector<EditsJob> with, without;
            for (const EditsJob &j : jobs) (j.lo ? with : without).push_back(j);
            Args b = a;
            F::set_width(b, e, vit);
            if (!without.empty() && edits_run<typename U::Rec>(e, without, F::template as<false>(a), vit, tiled, budget, t)) return -1;
            if (!with.empty() && edits_run<Rec>(e, with, b, vit, tiled, budget, t)) return -1;
            return 0;
        }
    }
};

/* private (scratch) bytes per lane of each banded form as the runtime reports them for the loaded code object, indexed as the form counts (the
 * combining kernel once per width of F::widths); -1: no answer */
template <class F>
static void edits_band_scratch(long long *bytes) {
    auto of = [](auto k) {
        hipFuncAttributes fa;
        return hipFuncGetAttributes(&fa, (const void *)decltype(k)::value) == hipSuccess ? (int)fa.localSizeBytes : -1;
    };
    for (int k = 0; bytes && k < 8; k++) bytes[k] = F::template rows<true>(of, (k & 4) != 0, (k & 2) != 0, (k & 1) != 0);
    for (size_t w = 0; bytes && w < sizeof(F::widths) / sizeof(int); w++)
        for (int k = 0; k < 4; k++) bytes[8 + 4 * w + k] = F::template edits<true>(of, (k & 2) != 0, (k & 1) != 0, F::widths[w]);
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
/* the tail of both per-read symbols of a family, after the checks of the matrix that u holds: the target's checks in the form's words -- where one
 * fails every score stays NAN, the reason is the error text and the answer 0 --, then edits_one on the form's arguments */
template <class F, bool BAND, class Upload>
static int edits_one_of(const char *fn, const EditsJob &job, const typename F::template Args<false> &u, bool vit, Upload &&upload) {
    using T = EditsForm<F, BAND>;
    const typename T::Args a = F::template as<BAND>(u);
    const scrappie_hip_map_target tg{job.seq, job.L, job.lo, job.hi};
    std::string why = T::target_why(tg, a);
    if (why.empty()) why = T::read_why(tg, job.nblock, a);
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }
    return edits_one<typename T::Rec>(job, a, vit, [&](scrappie_hip_engine *e, typename T::Args &up) {
        if constexpr (BAND) F::set_width(up, e, vit);
        return upload(e, up);
    });
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
    if (c.open(model, p, [&](Model *md) { return T::model_ok(fn, md); })) return -1;
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
