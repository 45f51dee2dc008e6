/* sh_eng_crf_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * every single-base edit of a sequence scored against a read of a flip-flop (CRF) model (k_crf_edits_rows, k_crf_edits, sh_crf_edits.h).
 * scrappie_hip_map_crf_edits_batch: the network and k_crf<true> of a launch group once, then the three kernels on the transitions where k_crf left
 * them in d_E; map_crf_edits: the same on a host matrix and the process-default engine.  Both run through sh_eng_edits.inc; the debug option
 * "crf_edits_budget_kb" cuts a launch group's reads into several launches.  What is here is the family's own, as an EditsTraits: the checks a
 * target and a model pass, the record's fields, the LDS of its kernels and their forms.  The layout of a launch's buffers is
 * scrappie_hip_crf_edits_plan's (sh_host.c). */

template <> struct EditsTraits<ShCrfEditsRead> {
    using Args = ShCrfEditsArgs;
    static constexpr const char *name = "map_crf_edits";
    static constexpr bool base_as_is = false;
    static EditsState &state(scrappie_hip_engine *e) { return e->crf_edits; }
    static size_t del_from(const Args &) { return 2; }       /* (the deletion of an only base leaves no sequence) */
    static long long plan(const size_t *L, const size_t *nblock, size_t n, const Args &, int *pitch, long long *rows, long long *res, long long *res_floats) {
        return scrappie_hip_crf_edits_plan(L, nblock, n, pitch, rows, res, res_floats);
    }
    static size_t read_bytes(size_t L, size_t nblock, const Args &) {
        return scrappie_hip_crf_edits_row_bytes(L, nblock) + (9 * L + 8) * 4 + L * 4 + sizeof(ShCrfEditsRead) + 64;
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
    static std::string target_why(const scrappie_hip_map_target &t, const Args &) {
        if (t.poslow || t.poshigh) return "bands are not part of this call";
        if (t.seqlen == 0) return "an empty sequence";
        if (!t.seq) return "no sequence";
        const size_t maxL = scrappie_hip_map_crf_lds_max_seq();
        if (t.seqlen > maxL) return "a sequence of " + std::to_string(t.seqlen) + " bases is too long for k_crf_edits (" + std::to_string(maxL) + ": score a window of it)";
        const size_t i = first_non_base(t.seq, t.seqlen);
        if (i < t.seqlen) return non_base_text(t.seq, i);
        return std::string();
    }
    static int model_ok(Model *m) {
        return m->arch != 1 ? set_err("map_crf_edits_batch: model '%s' is a transducer model; edits are scored for reads of flip-flop (CRF) models only", m->name.c_str()) : 0;
    }
    static Args args(const Model *, const scrappie_hip_params *, const RunOut &ro) {
        Args a{};
        a.trans = ro.E;
        return a;
    }
};

extern "C" void scrappie_hip_crf_edits_form_counts(uint64_t forms[12]) { edits_form_counts<ShCrfEditsRead>(forms); }
extern "C" void scrappie_hip_crf_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes) {
    if (e) edits_timing(e->crf_edits, ms, launches, row_bytes);
}

extern "C" int map_crf_edits(const_scrappie_matrix tr, const int *seq, size_t seqlen, int viterbi, float *base, float *sub, float *del, float *ins) {
    const char *const fn = "map_crf_edits";
    edits_nan(seq, seqlen, base, sub, del, ins);
    if (!tr || (!seq && seqlen)) return set_err("%s: null argument", fn);
    if (!sh_crf_post_ok(tr)) return set_err("%s: not a transition matrix of 25 rows and at least one block", fn);
    if (tr->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, tr->nc);
    const std::string why = EditsTraits<ShCrfEditsRead>::target_why(scrappie_hip_map_target{seq, seqlen, nullptr, nullptr}, ShCrfEditsArgs{});
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }      /* every score NAN, the reason as the error text */
    return edits_one<ShCrfEditsRead>(EditsJob{0, (int)tr->stride, tr->nc, seq, seqlen, base, sub, del, ins}, ShCrfEditsArgs{}, viterbi != 0,
                                     [&](scrappie_hip_engine *e, ShCrfEditsArgs &a) { return (a.trans = post_upload_trans(e, fn, tr)) ? 0 : -1; });
}

extern "C" int scrappie_hip_map_crf_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                                const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShCrfEditsRead>("map_crf_edits_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}
