/* sh_eng_map_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * every single-base edit of a sequence scored against a read of a transducer model (k_map_edits_rows, k_map_edits, sh_map_edits.h).
 * scrappie_hip_map_edits_batch: the network and S1 of a launch group once, then the three kernels on the posterior where S1 left it in d_E;
 * map_post_edits: the same on a host posterior and the process-default engine.  Both run through sh_eng_edits.inc; the debug option
 * "map_edits_budget_kb" cuts a launch group's reads into several launches.  What is here is the family's own, as an EditsTraits: the checks a
 * target and a model pass, the k-mer states of a read's bases, the record's fields, the LDS of its kernels and their forms.  The layout of a
 * launch's buffers is scrappie_hip_map_edits_plan's (sh_host.c).
 * scrappie_hip_map_edits_banded_batch and map_post_edits_banded: the same in a band, through the kernels' banded forms -- a second EditsTraits, on the
 * record with the band; its launches are laid out by scrappie_hip_map_edits_band_plan, count as their own forms and share the engine's EditsState,
 * budget and timing.  A target without a band in such a call takes the unbanded forms.  The debug option "map_edits_band_width" chooses the positions
 * per workgroup of the banded k_map_edits (64 or 256; 0: the default of the form, map_edits_band_default_width). */

/* k of a posterior of nr = 4^k + 1 rows, 1 .. SH_ME_K; 0: none */
static int map_edits_kmer(size_t nr) {
    size_t states = 4;
    for (int k = 1; k <= SH_ME_K; k++, states *= 4)
        if (nr == states + 1) return k;
    return 0;
}
/* dynamic LDS of k_map_edits: two buffers of SH_ME_CH columns */
static size_t map_edits_col_lds(size_t nr) { return 2 * (size_t)SH_ME_CH * ((nr + 3) & ~(size_t)3) * 4; }

template <> struct EditsTraits<ShMapEditsRead> {
    using Args = ShMapEditsArgs;
    static constexpr const char *name = "map_edits";
    static constexpr bool base_as_is = true;                 /* k_map's score as it is */
    static EditsState &state(scrappie_hip_engine *e) { return e->map_edits; }
    static size_t del_from(const Args &a) { return (size_t)a.k + 1; }      /* (a deletion from k bases leaves no state) */
    static long long plan(const EditsJob *, const size_t *L, const size_t *nblock, size_t n, const Args &a, int *pitch, long long *rows, long long *res, long long *res_floats) {
        return scrappie_hip_map_edits_plan(L, nblock, n, (size_t)a.k, pitch, rows, res, res_floats);
    }
    static size_t read_bytes(const EditsJob &j, const Args &a) {
        return scrappie_hip_map_edits_row_bytes(j.L, (size_t)a.k, j.nblock) + (9 * j.L + 8) * 4 + 2 * j.L * 4 + sizeof(ShMapEditsRead) + 64;
    }
    static std::string read_why(const scrappie_hip_map_target &, size_t, const Args &) { return std::string(); }
    static int run(scrappie_hip_engine *e, const std::vector<EditsJob> &jobs, const Args &a, bool vit, bool tiled, size_t budget, double *t) {
        return edits_run<ShMapEditsRead>(e, jobs, a, vit, tiled, budget, t);
    }
    static void fill(ShMapEditsRead &r, const EditsJob &j, std::vector<int> &codes, const Args &a) {
        const size_t K = (size_t)a.k;
        r.post = j.at; r.nbase = (int)j.L; r.seq = (long long)codes.size();
        unsigned code = 0;                                   /* the k-mer states, the oldest base the most significant (encode_bases_to_integers) */
        const unsigned mask = K >= 16 ? ~0u : (1u << (2 * K)) - 1u;
        for (size_t i = 0; i < j.L; i++) {
            code = ((code << 2) | (unsigned)j.seq[i]) & mask;
            if (i + 1 >= K) codes.push_back((int)code);
        }
        r.bases = (long long)codes.size();
        codes.insert(codes.end(), j.seq, j.seq + j.L);
    }
    static size_t lds_rows(size_t maxL, const Args &a) { return map_lds_bytes(maxL - (size_t)a.k + 1); }
    static size_t lds_edits(const Args &a) { return map_edits_col_lds((size_t)a.nr); }
    static int lds_err(size_t rows, size_t edits) { return set_err("map_edits: %zu and %zu bytes of LDS", rows, edits); }
    static int launch_rows(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled, bool back) {
        return pick_bool([&](auto v, auto tl, auto bk) { return launch_k<k_map_edits_rows<v(), tl(), bk()>>(grid, dim3(SH_MAP_NTH), lds, s, a); }, vit, tiled, back);
    }
    static int launch_edits(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled) {
        return pick_bool([&](auto v, auto tl) { return launch_k<k_map_edits<v(), tl()>>(grid, dim3(SH_MAP_NTH), lds, s, a); }, vit, tiled);
    }
    /* what a sequence must be, with a band or without */
    static std::string seq_why(const scrappie_hip_map_target &t, int k) {
        Args a{};
        a.k = k;
        scrappie_hip_map_target u = t;
        u.poslow = u.poshigh = nullptr;
        return target_why(u, a);
    }
    static std::string target_why(const scrappie_hip_map_target &t, const Args &a) {
        if (t.poslow || t.poshigh) return "bands are not part of this call";
        if (t.seqlen == 0) return "an empty sequence";
        if (!t.seq) return "no sequence";
        if (t.seqlen < (size_t)a.k) return "a sequence of " + std::to_string(t.seqlen) + " bases is shorter than the model's k-mer (" + std::to_string(a.k) + ")";
        const size_t maxL = scrappie_hip_map_edits_max_bases((size_t)a.k);
        if (t.seqlen > maxL) return "a sequence of " + std::to_string(t.seqlen) + " bases is too long for k_map_edits (" + std::to_string(maxL) + ": score a window of it)";
        const size_t i = first_non_base(t.seq, t.seqlen);
        if (i < t.seqlen) return non_base_text(t.seq, i);
        return std::string();
    }
    static int model_ok(Model *m) {
        if (m->arch == 1)
            return set_err("map_edits_batch: model '%s' is a flip-flop (CRF) model; its edits are scored with scrappie_hip_map_crf_edits_batch", m->name.c_str());
        if (!map_edits_kmer((size_t)m->NS)) return set_err("map_edits_batch: model '%s' has %d states, not 4^k + 1 for k = 1 .. %d", m->name.c_str(), m->NS, SH_ME_K);
        return ((m->NS + 3) / 4 - 1) / 4 < m->ff_mtiles ? 0 : set_err("map_edits_batch: model '%s' has %d states in %d chunks of 16", m->name.c_str(), m->NS, m->ff_mtiles);
    }
    static Args args(const Model *m, const scrappie_hip_params *p, const RunOut &ro) {
        Args a{};
        a.E = ro.E; a.sums = ro.sums; a.nr = m->NS; a.nchunk = m->ff_mtiles; a.k = map_edits_kmer((size_t)m->NS); a.min_prob = p->min_prob;
        a.stay_pen = p->stay_pen; a.skip_pen = p->skip_pen; a.local_pen = p->local_pen;
        return a;
    }
};

/* positions per workgroup of the banded k_map_edits: per form the faster of 64 and 256 in the path band of half-width 32 -- 64 in both, by 36 % (Viterbi)
 * and 61 % (forward) of the three kernels' time (profiles/map_edits_band_rate.txt).  The form is a parameter so that a later measurement can part
 * them; today both forms take the same width and there is no branch to look for. */
static int map_edits_band_default_width(bool) { return 64; }
static int map_edits_band_width(const scrappie_hip_engine *e, bool vit) { return e->map_edits_band_width ? e->map_edits_band_width : map_edits_band_default_width(vit); }
/* launches of the banded k_map_edits at 64 positions per workgroup, at (vit ? 2 : 0) | (tiled ? 1 : 0): g_edits_forms counts both widths */
static std::atomic<uint64_t> g_map_edits_band_w64[4];

/* In a band: the record carries the band's offset, the band travels as int32 behind the read's codes, the rows are the band's cells. */
template <> struct EditsTraits<ShMapEditsBandRead> {
    using Args = ShMapEditsBandArgs;
    using U = EditsTraits<ShMapEditsRead>;
    static constexpr const char *name = "map_edits_banded";
    static constexpr bool base_as_is = true;                 /* the masked programme's score as the kernel wrote it, as U's */
    static EditsState &state(scrappie_hip_engine *e) { return e->map_edits; }
    static ShMapEditsArgs plain(const Args &a) {             /* what the unbanded forms take of it */
        ShMapEditsArgs u{};
        u.post = a.post; u.E = a.E; u.sums = a.sums; u.pstride = a.pstride; u.nr = a.nr; u.nchunk = a.nchunk; u.k = a.k; u.min_prob = a.min_prob;
        u.stay_pen = a.stay_pen; u.skip_pen = a.skip_pen; u.local_pen = a.local_pen;
        return u;
    }
    static Args banded(const ShMapEditsArgs &u, int width) {
        Args a{};
        a.post = u.post; a.E = u.E; a.sums = u.sums; a.pstride = u.pstride; a.nr = u.nr; a.nchunk = u.nchunk; a.k = u.k; a.min_prob = u.min_prob;
        a.stay_pen = u.stay_pen; a.skip_pen = u.skip_pen; a.local_pen = u.local_pen; a.width = width;
        return a;
    }
    static size_t del_from(const Args &a) { return (size_t)a.k + 1; }
    static long long plan(const EditsJob *jobs, const size_t *L, const size_t *nblock, size_t n, const Args &a, int *pitch, long long *rows, long long *res, long long *res_floats) {
        std::vector<const size_t *> lo(n), hi(n);
        for (size_t k = 0; k < n; k++) { lo[k] = jobs[k].lo; hi[k] = jobs[k].hi; }
        return scrappie_hip_map_edits_band_plan(L, nblock, lo.data(), hi.data(), n, (size_t)a.k, pitch, rows, res, res_floats);
    }
    /* (a job without a band: what it costs the unbanded launch it goes to) */
    static size_t read_bytes(const EditsJob &j, const Args &a) {
        if (!j.lo || !j.hi) return U::read_bytes(j, plain(a));
        return scrappie_hip_map_edits_band_row_bytes(j.lo, j.hi, j.nblock) + (9 * j.L + 8) * 4 + 2 * j.L * 4 + 2 * j.nblock * 4 + sizeof(ShMapEditsBandRead) + 64;
    }
    static void fill(ShMapEditsBandRead &r, const EditsJob &j, std::vector<int> &codes, const Args &a) {
        U::fill(r, j, codes, plain(a));
        r.band = (long long)codes.size();
        for (const size_t *b : {j.lo, j.hi})
            for (size_t t = 0; t < j.nblock; t++) codes.push_back((int)b[t]);
    }
    static size_t lds_rows(size_t maxL, const Args &a) { return map_lds_bytes(maxL - (size_t)a.k + 1); }
    static size_t lds_edits(const Args &a) { return map_edits_col_lds((size_t)a.nr); }
    static int lds_err(size_t rows, size_t edits) { return set_err("map_edits_banded: %zu and %zu bytes of LDS", rows, edits); }
    static int launch_rows(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled, bool back) {
        return pick_bool([&](auto v, auto tl, auto bk) { return launch_k<k_map_edits_rows<v(), tl(), bk(), true>>(grid, dim3(SH_MAP_NTH), lds, s, a); }, vit, tiled, back);
    }
    /* (grid.y: chunks of SH_MAP_NTH positions; at 64 per workgroup four times as many, and a workgroup past the sequence returns) */
    static int launch_edits(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled) {
        if (a.width != 64) return pick_bool([&](auto v, auto tl) { return launch_k<k_map_edits<v(), tl(), true, SH_MAP_NTH>>(grid, dim3(SH_MAP_NTH), lds, s, a); }, vit, tiled);
        g_map_edits_band_w64[(vit ? 2 : 0) | (tiled ? 1 : 0)].fetch_add(1, std::memory_order_relaxed);
        return pick_bool([&](auto v, auto tl) { return launch_k<k_map_edits<v(), tl(), true, 64>>(dim3(grid.x, grid.y * (SH_MAP_NTH / 64)), dim3(64), lds, s, a); }, vit, tiled);
    }
    static std::string target_why(const scrappie_hip_map_target &t, const Args &a) {
        if (!t.poslow != !t.poshigh) return "a band needs both poslow and poshigh";
        return U::seq_why(t, a.k);
    }
    static std::string read_why(const scrappie_hip_map_target &t, size_t nblock, const Args &a) {
        const size_t n = t.seqlen - (size_t)a.k + 1;
        if (t.poslow && !sh_bounds_sane(t.poslow, t.poshigh, nblock, n, 0))
            return "the bands are not valid for a read of " + std::to_string(nblock) + " blocks and " + std::to_string(n) + " states (are_bounds_sane, " + std::to_string(nblock) + " entries each)";
        return std::string();
    }
    static int model_ok(Model *m) {
        if (m->arch == 1)
            return set_err("map_edits_banded_batch: model '%s' is a flip-flop (CRF) model; its edits are scored with scrappie_hip_map_crf_edits_banded_batch", m->name.c_str());
        if (!map_edits_kmer((size_t)m->NS)) return set_err("map_edits_banded_batch: model '%s' has %d states, not 4^k + 1 for k = 1 .. %d", m->name.c_str(), m->NS, SH_ME_K);
        return ((m->NS + 3) / 4 - 1) / 4 < m->ff_mtiles ? 0 : set_err("map_edits_banded_batch: model '%s' has %d states in %d chunks of 16", m->name.c_str(), m->NS, m->ff_mtiles);
    }
    static Args args(const Model *m, const scrappie_hip_params *p, const RunOut &ro) { return banded(U::args(m, p, ro), 0); }
    /* the jobs with a band through the banded forms at the engine's width, those without through the unbanded ones, each under the budget */
    static int run(scrappie_hip_engine *e, const std::vector<EditsJob> &jobs, const Args &a, bool vit, bool tiled, size_t budget, double *t) {
        std::vector<EditsJob> with, without;
        for (const EditsJob &j : jobs) (j.lo ? with : without).push_back(j);
        Args b = a;
        b.width = map_edits_band_width(e, vit);
        if (!without.empty() && edits_run<ShMapEditsRead>(e, without, plain(a), vit, tiled, budget, t)) return -1;
        if (!with.empty() && edits_run<ShMapEditsBandRead>(e, with, b, vit, tiled, budget, t)) return -1;
        return 0;
    }
};

extern "C" void scrappie_hip_map_edits_form_counts(uint64_t forms[12]) { edits_form_counts<ShMapEditsRead>(forms); }
/* the banded forms: [0..8) the rows kernel as above, [8..12) k_map_edits at 256 positions per workgroup, [12..16) at 64, each at (vit ? 2 : 0) | (tiled ? 1 : 0) */
extern "C" void scrappie_hip_map_edits_band_form_counts(uint64_t forms[16]) {
    if (!forms) return;
    edits_form_counts<ShMapEditsBandRead>(forms);
    for (int k = 0; k < 4; k++) {
        forms[12 + k] = g_map_edits_band_w64[k].load(std::memory_order_relaxed);
        forms[8 + k] -= std::min(forms[8 + k], forms[12 + k]);
    }
}
/* private (scratch) bytes per lane of each banded form as the runtime reports them for the loaded code object, indexed as the form counts; -1: no answer */
extern "C" void scrappie_hip_map_edits_band_scratch(long long bytes[16]) {
    auto of = [](const void *k) {
        hipFuncAttributes fa;
        return hipFuncGetAttributes(&fa, k) == hipSuccess ? (int)fa.localSizeBytes : -1;
    };
    for (int k = 0; bytes && k < 8; k++)
        bytes[k] = pick_bool([&](auto v, auto tl, auto bk) { return of((const void *)k_map_edits_rows<v(), tl(), bk(), true>); }, (k & 4) != 0, (k & 2) != 0, (k & 1) != 0);
    for (int k = 0; bytes && k < 4; k++) {
        bytes[8 + k] = pick_bool([&](auto v, auto tl) { return of((const void *)k_map_edits<v(), tl(), true, SH_MAP_NTH>); }, (k & 2) != 0, (k & 1) != 0);
        bytes[12 + k] = pick_bool([&](auto v, auto tl) { return of((const void *)k_map_edits<v(), tl(), true, 64>); }, (k & 2) != 0, (k & 1) != 0);
    }
}
extern "C" void scrappie_hip_map_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes) {
    if (e) edits_timing(e->map_edits, ms, launches, row_bytes);
}

/* the head both per-read symbols share: everything NAN, then the checks of the posterior, which a takes; 0: go on */
static int map_edits_one_head(const char *fn, const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, bool null_band,
                              float *base, float *sub, float *del, float *ins, ShMapEditsArgs &a) {
    edits_nan(seq, seqlen, base, sub, del, ins);
    if (!lp || (!seq && seqlen) || null_band) return set_err("%s: null argument", fn);
    a.pstride = (long long)lp->stride; a.nr = (int)lp->nr; a.k = map_edits_kmer(lp->nr);
    a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
    if (!a.k) return set_err("%s: a posterior of %zu rows is not 4^k + 1 states for k = 1 .. %d", fn, lp->nr, SH_ME_K);
    if (lp->nc == 0) return set_err("%s: a posterior of no blocks", fn);
    if (lp->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, lp->nc);
    if (lp->stride % 4 != 0 || lp->stride < ((lp->nr + 3) & ~(size_t)3))
        return set_err("%s: a posterior whose columns are %zu floats apart (whole 16-byte pieces of %zu states)", fn, lp->stride, lp->nr);
    return 0;
}

extern "C" int map_post_edits(const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, int viterbi, float *base,
                              float *sub, float *del, float *ins) {
    const char *const fn = "map_post_edits";
    ShMapEditsArgs a{};
    if (map_edits_one_head(fn, lp, stay_pen, skip_pen, local_pen, seq, seqlen, false, base, sub, del, ins, a)) return -1;
    const std::string why = EditsTraits<ShMapEditsRead>::target_why(scrappie_hip_map_target{seq, seqlen, nullptr, nullptr}, a);
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }      /* every score NAN, the reason as the error text */
    return edits_one<ShMapEditsRead>(EditsJob{0, 0, lp->nc, seq, seqlen, base, sub, del, ins}, a, viterbi != 0,
                                     [&](scrappie_hip_engine *e, ShMapEditsArgs &up) { return (up.post = post_upload_dense(e, fn, lp)) ? 0 : -1; });
}

extern "C" int map_post_edits_banded(const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, const size_t *low,
                                     const size_t *high, int viterbi, float *base, float *sub, float *del, float *ins) {
    using T = EditsTraits<ShMapEditsBandRead>;
    const char *const fn = "map_post_edits_banded";
    ShMapEditsArgs u{};
    if (map_edits_one_head(fn, lp, stay_pen, skip_pen, local_pen, seq, seqlen, !low || !high, base, sub, del, ins, u)) return -1;
    const ShMapEditsBandArgs a = T::banded(u, 0);
    const scrappie_hip_map_target tg{seq, seqlen, low, high};
    std::string why = T::target_why(tg, a);
    if (why.empty()) why = T::read_why(tg, lp->nc, a);
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }
    return edits_one<ShMapEditsBandRead>(EditsJob{0, 0, lp->nc, seq, seqlen, base, sub, del, ins, low, high}, a, viterbi != 0,
                                         [&](scrappie_hip_engine *e, ShMapEditsBandArgs &up) {
                                             up.width = map_edits_band_width(e, viterbi != 0);
                                             return (up.post = post_upload_dense(e, fn, lp)) ? 0 : -1;
                                         });
}

extern "C" int scrappie_hip_map_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                            const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShMapEditsRead>("map_edits_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}

extern "C" int scrappie_hip_map_edits_banded_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                                   const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShMapEditsBandRead>("map_edits_banded_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}
