/* sh_eng_crf_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * every single-base edit of a sequence scored against a read of a flip-flop (CRF) model (k_crf_edits_rows, k_crf_edits, sh_crf_edits.h).
 * scrappie_hip_map_crf_edits_batch: the network and k_crf<true> of a launch group once, then the three kernels on the transitions where k_crf left
 * them in d_E; map_crf_edits: the same on a host matrix and the process-default engine.  Both run through sh_eng_edits.inc; the debug option
 * "crf_edits_budget_kb" cuts a launch group's reads into several launches.  What is here is the family's own, said once for both forms (CrfEdits, as
 * EditsForm reads it): the checks a sequence, a band and a model pass, the record's fields, the LDS of its kernels and their forms.  The layout of a
 * launch's buffers is scrappie_hip_crf_edits_plan's (sh_host.c).
 * scrappie_hip_map_crf_edits_banded_batch and map_crf_edits_banded: the same in a band, through the kernels' banded forms and EditsForm<CrfEdits,
 * true>; its launches are laid out by scrappie_hip_crf_edits_band_plan, count as their own forms and share the engine's EditsState, budget and
 * timing.  A target without a band in such a call takes the unbanded forms. */

struct CrfEdits : EditsOneWidth {
    template <bool BAND> using Rec = std::conditional_t<BAND, ShCrfEditsBandRead, ShCrfEditsRead>;
    template <bool BAND> using Args = ShCrfEditsArgsOf<BAND>;
    static constexpr const char *name[2] = {"map_crf_edits", "map_crf_edits_banded"};
    static constexpr bool base_as_is = false;
    static constexpr size_t code_ints = 1;                   /* the base codes */
    static EditsState &state(scrappie_hip_engine *e) { return e->crf_edits; }
    template <class A> static size_t del_from(const A &) { return 2; }       /* (the deletion of an only base leaves no sequence) */
    template <bool BAND, class A>
    static long long plan(const size_t *L, const size_t *nblock, const size_t *const *lo, const size_t *const *hi, size_t n, const A &, int *pitch, long long *rows, long long *res, long long *res_floats) {
        return BAND ? scrappie_hip_crf_edits_band_plan(L, nblock, lo, hi, n, pitch, rows, res, res_floats) : scrappie_hip_crf_edits_plan(L, nblock, n, pitch, rows, res, res_floats);
    }
    template <class A> static size_t row_bytes(const EditsJob &j, const A &) { return scrappie_hip_crf_edits_row_bytes(j.L, j.nblock); }
    template <class A> static void fill(ShCrfEditsRead &r, const EditsJob &j, std::vector<int> &codes, const A &) {
        r.trans = j.at; r.seqlen = (int)j.L; r.seq = (long long)codes.size();
        codes.insert(codes.end(), j.seq, j.seq + j.L);
    }
    template <class A> static size_t lds_rows(size_t maxL, const A &) { return map_crf_lds_bytes(maxL); }
    template <class A> static size_t lds_edits(const A &) { return 0; }
    static int lds_err(const char *fn, size_t rows, size_t) { return set_err("%s: rows of %zu bytes of LDS", fn, rows); }
    template <class A> static std::string seq_why(const scrappie_hip_map_target &t, const A &) {
        if (t.seqlen == 0) return "an empty sequence";
        if (!t.seq) return "no sequence";
        const size_t maxL = scrappie_hip_map_crf_lds_max_seq();
        if (t.seqlen > maxL) return "a sequence of " + std::to_string(t.seqlen) + " bases is too long for k_crf_edits (" + std::to_string(maxL) + ": score a window of it)";
        const size_t i = first_non_base(t.seq, t.seqlen);
        if (i < t.seqlen) return non_base_text(t.seq, i);
        return std::string();
    }
    static int model_ok(const char *fn, bool, Model *m) {
        return m->arch != 1 ? set_err("%s: model '%s' is a transducer model; edits are scored for reads of flip-flop (CRF) models only", fn, m->name.c_str()) : 0;
    }
    static Args<false> args(const Model *, const scrappie_hip_params *, const RunOut &ro) {
        Args<false> a{};
        a.trans = ro.E;
        return a;
    }
    template <bool BAND, class A> static Args<BAND> as(const A &u) {
        Args<BAND> a{};
        a.trans = u.trans;
        return a;
    }
    static size_t band_entries(size_t nblock) { return nblock + 1; }
    static size_t band_row_bytes(const size_t *lo, const size_t *hi, size_t nblock) { return scrappie_hip_crf_edits_band_row_bytes(lo, hi, nblock); }
    template <class A> static std::string band_why(const scrappie_hip_map_target &t, size_t nblock, const A &) {
        if (scrappie_hip_map_crf_bounds_sane(t.poslow, t.poshigh, nblock, t.seqlen)) return std::string();
        return "the bands are not valid for a read of " + std::to_string(nblock) + " blocks (scrappie_hip_map_crf_bounds_sane, " + std::to_string(nblock + 1) + " entries each)";
    }
    template <bool BAND, class Fn> static int rows(Fn &&f, bool vit, bool tiled, bool back) {
        return pick_bool([&](auto v, auto tl, auto bk) { return f(kernel_c<k_crf_edits_rows<v(), std::conditional_t<tl(), ShCrfTiled, ShCrfRef>, bk(), BAND>>()); }, vit, tiled, back);
    }
    template <bool BAND, class Fn> static int edits(Fn &&f, bool vit, bool tiled, int) {
        return pick_bool([&](auto v, auto tl) { return f(kernel_c<k_crf_edits<v(), std::conditional_t<tl(), ShCrfTiled, ShCrfRef>, BAND>>()); }, vit, tiled);
    }
};
template <> struct EditsTraits<ShCrfEditsRead> : EditsForm<CrfEdits, false> {};
template <> struct EditsTraits<ShCrfEditsBandRead> : EditsForm<CrfEdits, true> {};

extern "C" void scrappie_hip_crf_edits_form_counts(uint64_t forms[12]) { edits_form_counts<ShCrfEditsRead>(forms); }
extern "C" void scrappie_hip_crf_edits_band_form_counts(uint64_t forms[12]) { edits_form_counts<ShCrfEditsBandRead>(forms); }
extern "C" void scrappie_hip_crf_edits_band_scratch(long long bytes[12]) { edits_band_scratch<CrfEdits>(bytes); }
extern "C" void scrappie_hip_crf_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes) {
    if (e) edits_timing(e->crf_edits, ms, launches, row_bytes);
}

/* both per-read symbols: everything NAN, the checks of the matrix, then the form's tail */
template <bool BAND>
static int crf_edits_one(const char *fn, const_scrappie_matrix tr, const int *seq, size_t seqlen, const size_t *low, const size_t *high, int viterbi,
                         float *base, float *sub, float *del, float *ins) {
    edits_nan(seq, seqlen, base, sub, del, ins);
    if (!tr || (!seq && seqlen) || (BAND && (!low || !high))) return set_err("%s: null argument", fn);
    if (!sh_crf_post_ok(tr)) return set_err("%s: not a transition matrix of 25 rows and at least one block", fn);
    if (tr->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, tr->nc);
    return edits_one_of<CrfEdits, BAND>(fn, EditsJob{0, (int)tr->stride, tr->nc, seq, seqlen, base, sub, del, ins, low, high}, ShCrfEditsArgs{}, viterbi != 0,
                                        [&](scrappie_hip_engine *e, auto &a) { return (a.trans = post_upload_trans(e, fn, tr)) ? 0 : -1; });
}
extern "C" int map_crf_edits(const_scrappie_matrix tr, const int *seq, size_t seqlen, int viterbi, float *base, float *sub, float *del, float *ins) {
    return crf_edits_one<false>("map_crf_edits", tr, seq, seqlen, nullptr, nullptr, viterbi, base, sub, del, ins);
}
extern "C" int map_crf_edits_banded(const_scrappie_matrix tr, const int *seq, size_t seqlen, const size_t *low, const size_t *high, int viterbi,
                                    float *base, float *sub, float *del, float *ins) {
    return crf_edits_one<true>("map_crf_edits_banded", tr, seq, seqlen, low, high, viterbi, base, sub, del, ins);
}

extern "C" int scrappie_hip_map_crf_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                                const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShCrfEditsRead>("map_crf_edits_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}

extern "C" int scrappie_hip_map_crf_edits_banded_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                                       const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShCrfEditsBandRead>("map_crf_edits_banded_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}
