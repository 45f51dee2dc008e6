/* sh_eng_crf_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * every single-base edit of a sequence scored against a read of a flip-flop (CRF) model (k_crf_edits_rows, k_crf_edits, sh_crf_edits.h).
 * scrappie_hip_map_crf_edits_batch: the network and k_crf<true> of a launch group once, then the three kernels on the transitions where k_crf left
 * them in d_E; map_crf_edits: the same on a host matrix and the process-default engine.  Both run through sh_eng_edits.inc; the debug option
 * "crf_edits_budget_kb" cuts a launch group's reads into several launches.  What is here is the family's own, as an EditsTraits: the checks a
 * target and a model pass, the record's fields, the LDS of its kernels and their forms.  The layout of a launch's buffers is
 * scrappie_hip_crf_edits_plan's (sh_host.c).
 * scrappie_hip_map_crf_edits_banded_batch and map_crf_edits_banded: the same in a band, through the kernels' banded forms -- a second EditsTraits, on
 * the record with the band; its launches are laid out by scrappie_hip_crf_edits_band_plan, count as their own forms and share the engine's
 * EditsState, budget and timing.  A target without a band in such a call takes the unbanded forms. */

template <> struct EditsTraits<ShCrfEditsRead> {
    using Args = ShCrfEditsArgs;
    static constexpr const char *name = "map_crf_edits";
    static constexpr bool base_as_is = false;
    static EditsState &state(scrappie_hip_engine *e) { return e->crf_edits; }
    static size_t del_from(const Args &) { return 2; }       /* (the deletion of an only base leaves no sequence) */
    static long long plan(const EditsJob *, const size_t *L, const size_t *nblock, size_t n, const Args &, int *pitch, long long *rows, long long *res, long long *res_floats) {
        return scrappie_hip_crf_edits_plan(L, nblock, n, pitch, rows, res, res_floats);
    }
    static size_t read_bytes(const EditsJob &j, const Args &) {
        return scrappie_hip_crf_edits_row_bytes(j.L, j.nblock) + (9 * j.L + 8) * 4 + j.L * 4 + sizeof(ShCrfEditsRead) + 64;
    }
    static void fill(ShCrfEditsRead &r, const EditsJob &j, std::vector<int> &codes, const Args &) {
        r.trans = j.at; r.seqlen = (int)j.L; r.seq = (long long)codes.size();
        codes.insert(codes.end(), j.seq, j.seq + j.L);
    }
    static size_t lds_rows(size_t maxL, const Args &) { return map_crf_lds_bytes(maxL); }
    static size_t lds_edits(const Args &) { return 0; }
    static int lds_err(size_t rows, size_t) { return set_err("map_crf_edits: rows of %zu bytes of LDS", rows); }
    static int launch_rows(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled, bool back) {
        return pick_bool([&](auto v, auto tl, auto bk) {
            return launch_k<k_crf_edits_rows<v(), std::conditional_t<tl(), ShCrfTiled, ShCrfRef>, bk()>>(grid, dim3(SH_MAP_NTH), lds, s, a);
        }, vit, tiled, back);
    }
    static int launch_edits(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled) {
        return pick_bool([&](auto v, auto tl) {
            return launch_k<k_crf_edits<v(), std::conditional_t<tl(), ShCrfTiled, ShCrfRef>>>(grid, dim3(SH_MAP_NTH), lds, s, a);
        }, vit, tiled);
    }
    /* what a sequence must be, with a band or without */
    static std::string seq_why(const scrappie_hip_map_target &t) {
        if (t.seqlen == 0) return "an empty sequence";
        if (!t.seq) return "no sequence";
        const size_t maxL = scrappie_hip_map_crf_lds_max_seq();
        if (t.seqlen > maxL) return "a sequence of " + std::to_string(t.seqlen) + " bases is too long for k_crf_edits (" + std::to_string(maxL) + ": score a window of it)";
        const size_t i = first_non_base(t.seq, t.seqlen);
        if (i < t.seqlen) return non_base_text(t.seq, i);
        return std::string();
    }
    static std::string target_why(const scrappie_hip_map_target &t, const Args &) {
        if (t.poslow || t.poshigh) return "bands are not part of this call";
        return seq_why(t);
    }
    static std::string read_why(const scrappie_hip_map_target &, size_t, const Args &) { return std::string(); }
    static int model_ok(Model *m) {
        return m->arch != 1 ? set_err("map_crf_edits_batch: model '%s' is a transducer model; edits are scored for reads of flip-flop (CRF) models only", m->name.c_str()) : 0;
    }
    static Args args(const Model *, const scrappie_hip_params *, const RunOut &ro) {
        Args a{};
        a.trans = ro.E;
        return a;
    }
    static int run(scrappie_hip_engine *e, const std::vector<EditsJob> &jobs, const Args &a, bool vit, bool tiled, size_t budget, double *t) {
        return edits_run<ShCrfEditsRead>(e, jobs, a, vit, tiled, budget, t);
    }
};

/* In a band: the record carries the band's offset, the band travels behind the read's codes, the rows are the band's cells. */
template <> struct EditsTraits<ShCrfEditsBandRead> {
    using Args = ShCrfEditsBandArgs;
    using U = EditsTraits<ShCrfEditsRead>;
    static constexpr const char *name = "map_crf_edits_banded";
    static constexpr bool base_as_is = false;
    static EditsState &state(scrappie_hip_engine *e) { return e->crf_edits; }
    static size_t del_from(const Args &) { return 2; }
    static long long plan(const EditsJob *jobs, const size_t *L, const size_t *nblock, size_t n, const Args &, int *pitch, long long *rows, long long *res, long long *res_floats) {
        std::vector<const size_t *> lo(n), hi(n);
        for (size_t k = 0; k < n; k++) { lo[k] = jobs[k].lo; hi[k] = jobs[k].hi; }
        return scrappie_hip_crf_edits_band_plan(L, nblock, lo.data(), hi.data(), n, pitch, rows, res, res_floats);
    }
    /* (a job without a band: what it costs the unbanded launch it goes to) */
    static size_t read_bytes(const EditsJob &j, const Args &) {
        if (!j.lo || !j.hi) return U::read_bytes(j, ShCrfEditsArgs{});
        return scrappie_hip_crf_edits_band_row_bytes(j.lo, j.hi, j.nblock) + (9 * j.L + 8) * 4 + j.L * 4 + 2 * (j.nblock + 1) * 4 + sizeof(ShCrfEditsBandRead) + 64;
    }
    static void fill(ShCrfEditsBandRead &r, const EditsJob &j, std::vector<int> &codes, const Args &) {
        U::fill(r, j, codes, ShCrfEditsArgs{});
        r.band = (long long)codes.size();
        for (const size_t *b : {j.lo, j.hi})
            for (size_t t = 0; t <= j.nblock; t++) codes.push_back((int)b[t]);
    }
    static size_t lds_rows(size_t maxL, const Args &) { return map_crf_lds_bytes(maxL); }
    static size_t lds_edits(const Args &) { return 0; }
    static int lds_err(size_t rows, size_t) { return set_err("map_crf_edits_banded: rows of %zu bytes of LDS", rows); }
    static int launch_rows(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled, bool back) {
        return pick_bool([&](auto v, auto tl, auto bk) {
            return launch_k<k_crf_edits_rows<v(), std::conditional_t<tl(), ShCrfTiled, ShCrfRef>, bk(), true>>(grid, dim3(SH_MAP_NTH), lds, s, a);
        }, vit, tiled, back);
    }
    static int launch_edits(dim3 grid, size_t lds, hipStream_t s, const Args &a, bool vit, bool tiled) {
        return pick_bool([&](auto v, auto tl) {
            return launch_k<k_crf_edits<v(), std::conditional_t<tl(), ShCrfTiled, ShCrfRef>, true>>(grid, dim3(SH_MAP_NTH), lds, s, a);
        }, vit, tiled);
    }
    static std::string target_why(const scrappie_hip_map_target &t, const Args &) {
        if (!t.poslow != !t.poshigh) return "a band needs both poslow and poshigh";
        return U::seq_why(t);
    }
    static std::string read_why(const scrappie_hip_map_target &t, size_t nblock, const Args &) {
        if (t.poslow && !scrappie_hip_map_crf_bounds_sane(t.poslow, t.poshigh, nblock, t.seqlen))
            return "the bands are not valid for a read of " + std::to_string(nblock) + " blocks (scrappie_hip_map_crf_bounds_sane, " + std::to_string(nblock + 1) + " entries each)";
        return std::string();
    }
    static int model_ok(Model *m) {
        return m->arch != 1 ? set_err("map_crf_edits_banded_batch: model '%s' is a transducer model; edits are scored for reads of flip-flop (CRF) models only", m->name.c_str()) : 0;
    }
    static Args args(const Model *, const scrappie_hip_params *, const RunOut &ro) {
        Args a{};
        a.trans = ro.E;
        return a;
    }
    /* the jobs with a band through the banded forms, those without through the unbanded ones, each under the budget */
    static int run(scrappie_hip_engine *e, const std::vector<EditsJob> &jobs, const Args &a, bool vit, bool tiled, size_t budget, double *t) {
        std::vector<EditsJob> with, without;
        for (const EditsJob &j : jobs) (j.lo ? with : without).push_back(j);
        ShCrfEditsArgs u{};
        u.trans = a.trans;
        if (!without.empty() && edits_run<ShCrfEditsRead>(e, without, u, vit, tiled, budget, t)) return -1;
        if (!with.empty() && edits_run<ShCrfEditsBandRead>(e, with, a, vit, tiled, budget, t)) return -1;
        return 0;
    }
};

extern "C" void scrappie_hip_crf_edits_form_counts(uint64_t forms[12]) { edits_form_counts<ShCrfEditsRead>(forms); }
extern "C" void scrappie_hip_crf_edits_band_form_counts(uint64_t forms[12]) { edits_form_counts<ShCrfEditsBandRead>(forms); }
/* private (scratch) bytes per lane of each banded form as the runtime reports them for the loaded code object, indexed as the form counts; -1: no answer */
extern "C" void scrappie_hip_crf_edits_band_scratch(long long bytes[12]) {
    auto of = [](const void *k) {
        hipFuncAttributes fa;
        return hipFuncGetAttributes(&fa, k) == hipSuccess ? (int)fa.localSizeBytes : -1;
    };
    for (int k = 0; bytes && k < 8; k++)
        bytes[k] = pick_bool([&](auto v, auto tl, auto bk) {
            return of((const void *)k_crf_edits_rows<v(), std::conditional_t<tl(), ShCrfTiled, ShCrfRef>, bk(), true>);
        }, (k & 4) != 0, (k & 2) != 0, (k & 1) != 0);
    for (int k = 0; bytes && k < 4; k++)
        bytes[8 + k] = pick_bool([&](auto v, auto tl) {
            return of((const void *)k_crf_edits<v(), std::conditional_t<tl(), ShCrfTiled, ShCrfRef>, true>);
        }, (k & 2) != 0, (k & 1) != 0);
}
extern "C" void scrappie_hip_crf_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes) {
    if (e) edits_timing(e->crf_edits, ms, launches, row_bytes);
}

/* the head both per-read symbols share: everything NAN, then the checks of the matrix; 0: go on */
static int crf_edits_one_head(const char *fn, const_scrappie_matrix tr, const int *seq, size_t seqlen, bool null_band, float *base, float *sub, float *del, float *ins) {
    edits_nan(seq, seqlen, base, sub, del, ins);
    if (!tr || (!seq && seqlen) || null_band) return set_err("%s: null argument", fn);
    if (!sh_crf_post_ok(tr)) return set_err("%s: not a transition matrix of 25 rows and at least one block", fn);
    if (tr->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, tr->nc);
    return 0;
}

extern "C" int map_crf_edits(const_scrappie_matrix tr, const int *seq, size_t seqlen, int viterbi, float *base, float *sub, float *del, float *ins) {
    const char *const fn = "map_crf_edits";
    if (crf_edits_one_head(fn, tr, seq, seqlen, false, base, sub, del, ins)) return -1;
    const std::string why = EditsTraits<ShCrfEditsRead>::target_why(scrappie_hip_map_target{seq, seqlen, nullptr, nullptr}, ShCrfEditsArgs{});
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }      /* every score NAN, the reason as the error text */
    return edits_one<ShCrfEditsRead>(EditsJob{0, (int)tr->stride, tr->nc, seq, seqlen, base, sub, del, ins, nullptr, nullptr}, ShCrfEditsArgs{}, viterbi != 0,
                                     [&](scrappie_hip_engine *e, ShCrfEditsArgs &a) { return (a.trans = post_upload_trans(e, fn, tr)) ? 0 : -1; });
}

extern "C" int map_crf_edits_banded(const_scrappie_matrix tr, const int *seq, size_t seqlen, const size_t *low, const size_t *high, int viterbi,
                                    float *base, float *sub, float *del, float *ins) {
    using T = EditsTraits<ShCrfEditsBandRead>;
    const char *const fn = "map_crf_edits_banded";
    if (crf_edits_one_head(fn, tr, seq, seqlen, !low || !high, base, sub, del, ins)) return -1;
    const scrappie_hip_map_target tg{seq, seqlen, low, high};
    std::string why = T::target_why(tg, ShCrfEditsBandArgs{});
    if (why.empty()) why = T::read_why(tg, tr->nc, ShCrfEditsBandArgs{});
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }
    return edits_one<ShCrfEditsBandRead>(EditsJob{0, (int)tr->stride, tr->nc, seq, seqlen, base, sub, del, ins, low, high}, ShCrfEditsBandArgs{}, viterbi != 0,
                                         [&](scrappie_hip_engine *e, ShCrfEditsBandArgs &a) { return (a.trans = post_upload_trans(e, fn, tr)) ? 0 : -1; });
}

extern "C" int scrappie_hip_map_crf_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                                const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShCrfEditsRead>("map_crf_edits_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}

extern "C" int scrappie_hip_map_crf_edits_banded_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                                       const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShCrfEditsBandRead>("map_crf_edits_banded_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}
