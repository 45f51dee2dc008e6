/* sh_eng_map_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * every single-base edit of a sequence scored against a read of a transducer model (k_map_edits_rows, k_map_edits, sh_map_edits.h).
 * scrappie_hip_map_edits_batch: the network and S1 of a launch group once, then the three kernels on the posterior where S1 left it in d_E;
 * map_post_edits: the same on a host posterior and the process-default engine.  Both run through sh_eng_edits.inc; the debug option
 * "map_edits_budget_kb" cuts a launch group's reads into several launches.  What is here is the family's own, said once for both forms (MapEdits, as
 * EditsForm reads it): the checks a sequence, a band and a model pass, the k-mer states of a read's bases, the record's fields, the LDS of its
 * kernels and their forms.  The layout of a launch's buffers is scrappie_hip_map_edits_plan's (sh_host.c).
 * scrappie_hip_map_edits_banded_batch and map_post_edits_banded: the same in a band, through the kernels' banded forms and EditsForm<MapEdits, true>;
 * its launches are laid out by scrappie_hip_map_edits_band_plan, count as their own forms and share the engine's EditsState, budget and timing.  A
 * target without a band in such a call takes the unbanded forms.  The debug option "map_edits_band_width" chooses the positions per workgroup of
 * the banded k_map_edits (64 or 256; 0: the default of the form, map_edits_band_default_width). */

/* k of a posterior of nr = 4^k + 1 rows, 1 .. SH_ME_K; 0: none */
static int map_edits_kmer(size_t nr) {
    size_t states = 4;
    for (int k = 1; k <= SH_ME_K; k++, states *= 4)
        if (nr == states + 1) return k;
    return 0;
}
/* dynamic LDS of k_map_edits: two buffers of SH_ME_CH columns */
static size_t map_edits_col_lds(size_t nr) { return 2 * (size_t)SH_ME_CH * ((nr + 3) & ~(size_t)3) * 4; }

/* positions per workgroup of the banded k_map_edits: per form the faster of 64 and 256 in the path band of half-width 32 -- 64 in both, by 36 % (Viterbi)
 * and 61 % (forward) of the three kernels' time (profiles/map_edits_band_rate.txt).  The form is a parameter so that a later measurement can part
 * them; today both forms take the same width and there is no branch to look for. */
static int map_edits_band_default_width(bool) { return 64; }
/* launches of the banded k_map_edits at 64 positions per workgroup, at (vit ? 2 : 0) | (tiled ? 1 : 0): g_edits_forms counts both widths */
static std::atomic<uint64_t> g_map_edits_band_w64[4];

struct MapEdits {
    template <bool BAND> using Rec = std::conditional_t<BAND, ShMapEditsBandRead, ShMapEditsRead>;
    template <bool BAND> using Args = ShMapEditsArgsOf<BAND>;
    static constexpr const char *name[2] = {"map_edits", "map_edits_banded"};
    static constexpr bool base_as_is = true;                 /* k_map's score, or the masked programme's, as the kernel wrote it */
    static constexpr size_t code_ints = 2;                   /* the k-mer states and the base codes */
    static constexpr int widths[2] = {SH_MAP_NTH, 64};
    static EditsState &state(scrappie_hip_engine *e) { return e->map_edits; }
    template <class A> static size_t del_from(const A &a) { return (size_t)a.k + 1; }      /* (a deletion from k bases leaves no state) */
    template <bool BAND, class A>
    static long long plan(const size_t *L, const size_t *nblock, const size_t *const *lo, const size_t *const *hi, size_t n, const A &a, int *pitch, long long *rows, long long *res, long long *res_floats) {
        return BAND ? scrappie_hip_map_edits_band_plan(L, nblock, lo, hi, n, (size_t)a.k, pitch, rows, res, res_floats)
                  : scrappie_hip_map_edits_plan(L, nblock, n, (size_t)a.k, pitch, rows, res, res_floats);
    }
    template <class A> static size_t row_bytes(const EditsJob &j, const A &a) { return scrappie_hip_map_edits_row_bytes(j.L, (size_t)a.k, j.nblock); }
    template <class A> static void fill(ShMapEditsRead &r, const EditsJob &j, std::vector<int> &codes, const A &a) {
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
    template <class A> static size_t lds_rows(size_t maxL, const A &a) { return map_lds_bytes(maxL - (size_t)a.k + 1); }
    template <class A> static size_t lds_edits(const A &a) { return map_edits_col_lds((size_t)a.nr); }
    static int lds_err(const char *fn, size_t rows, size_t edits) { return set_err("%s: %zu and %zu bytes of LDS", fn, rows, edits); }
    template <class A> static std::string seq_why(const scrappie_hip_map_target &t, const A &a) {
        if (t.seqlen == 0) return "an empty sequence";
        if (!t.seq) return "no sequence";
        if (t.seqlen < (size_t)a.k) return "a sequence of " + std::to_string(t.seqlen) + " bases is shorter than the model's k-mer (" + std::to_string(a.k) + ")";
        const size_t maxL = scrappie_hip_map_edits_max_bases((size_t)a.k);
        if (t.seqlen > maxL) return "a sequence of " + std::to_string(t.seqlen) + " bases is too long for k_map_edits (" + std::to_string(maxL) + ": score a window of it)";
        const size_t i = first_non_base(t.seq, t.seqlen);
        if (i < t.seqlen) return non_base_text(t.seq, i);
        return std::string();
    }
    static int model_ok(const char *fn, bool band, Model *m) {
        if (m->arch == 1)
            return set_err("%s: model '%s' is a flip-flop (CRF) model; its edits are scored with %s", fn, m->name.c_str(),
                           band ? "scrappie_hip_map_crf_edits_banded_batch" : "scrappie_hip_map_crf_edits_batch");
        if (!map_edits_kmer((size_t)m->NS)) return set_err("%s: model '%s' has %d states, not 4^k + 1 for k = 1 .. %d", fn, m->name.c_str(), m->NS, SH_ME_K);
        return ((m->NS + 3) / 4 - 1) / 4 < m->ff_mtiles ? 0 : set_err("%s: model '%s' has %d states in %d chunks of 16", fn, m->name.c_str(), m->NS, m->ff_mtiles);
    }
    static Args<false> args(const Model *m, const scrappie_hip_params *p, const RunOut &ro) {
        Args<false> a{};
        a.E = ro.E; a.sums = ro.sums; a.nr = m->NS; a.nchunk = m->ff_mtiles; a.k = map_edits_kmer((size_t)m->NS); a.min_prob = p->min_prob;
        a.stay_pen = p->stay_pen; a.skip_pen = p->skip_pen; a.local_pen = p->local_pen;
        return a;
    }
    template <bool BAND, class A> static Args<BAND> as(const A &u) { return sh_map_edits_args_as<Args<BAND>>(u); }
    static size_t band_entries(size_t nblock) { return nblock; }
    static size_t band_row_bytes(const size_t *lo, const size_t *hi, size_t nblock) { return scrappie_hip_map_edits_band_row_bytes(lo, hi, nblock); }
    template <class A> static std::string band_why(const scrappie_hip_map_target &t, size_t nblock, const A &a) {
        const size_t n = t.seqlen - (size_t)a.k + 1;
        if (sh_bounds_sane(t.poslow, t.poshigh, nblock, n, 0)) return std::string();
        return "the bands are not valid for a read of " + std::to_string(nblock) + " blocks and " + std::to_string(n) + " states (are_bounds_sane, " + std::to_string(nblock) + " entries each)";
    }
    template <bool BAND, class Fn> static int rows(Fn &&f, bool vit, bool tiled, bool back) {
        return pick_bool([&](auto v, auto tl, auto bk) { return f(kernel_c<k_map_edits_rows<v(), tl(), bk(), BAND>>()); }, vit, tiled, back);
    }
    template <bool BAND, class Fn> static int edits(Fn &&f, bool vit, bool tiled, int width) {
        if constexpr (BAND) if (width == 64) return pick_bool([&](auto v, auto tl) { return f(kernel_c<k_map_edits<v(), tl(), true, 64>>()); }, vit, tiled);
        return pick_bool([&](auto v, auto tl) { return f(kernel_c<k_map_edits<v(), tl(), BAND, SH_MAP_NTH>>()); }, vit, tiled);
    }
    /* the banded combining kernel at the engine's width (host only: ShMapEditsBandArgs::width); everything else at SH_MAP_NTH */
    static void set_width(ShMapEditsBandArgs &a, const scrappie_hip_engine *e, bool vit) { a.width = e->map_edits_band_width ? e->map_edits_band_width : map_edits_band_default_width(vit); }
    static int width_of(const ShMapEditsArgs &) { return SH_MAP_NTH; }
    static int width_of(const ShMapEditsBandArgs &a) { return a.width == 64 ? 64 : SH_MAP_NTH; }
    static void count_width(int width, bool vit, bool tiled) { if (width == 64) g_map_edits_band_w64[(vit ? 2 : 0) | (tiled ? 1 : 0)].fetch_add(1, std::memory_order_relaxed); }
};
template <> struct EditsTraits<ShMapEditsRead> : EditsForm<MapEdits, false> {};
template <> struct EditsTraits<ShMapEditsBandRead> : EditsForm<MapEdits, true> {};

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
extern "C" void scrappie_hip_map_edits_band_scratch(long long bytes[16]) { edits_band_scratch<MapEdits>(bytes); }
extern "C" void scrappie_hip_map_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes) {
    if (e) edits_timing(e->map_edits, ms, launches, row_bytes);
}

/* both per-read symbols: everything NAN, the checks of the posterior, then the form's tail */
template <bool BAND>
static int map_edits_one(const char *fn, const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, const size_t *low,
                         const size_t *high, int viterbi, float *base, float *sub, float *del, float *ins) {
    edits_nan(seq, seqlen, base, sub, del, ins);
    if (!lp || (!seq && seqlen) || (BAND && (!low || !high))) return set_err("%s: null argument", fn);
    ShMapEditsArgs a{};
    a.pstride = (long long)lp->stride; a.nr = (int)lp->nr; a.k = map_edits_kmer(lp->nr);
    a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
    if (!a.k) return set_err("%s: a posterior of %zu rows is not 4^k + 1 states for k = 1 .. %d", fn, lp->nr, SH_ME_K);
    if (lp->nc == 0) return set_err("%s: a posterior of no blocks", fn);
    if (lp->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, lp->nc);
    if (lp->stride % 4 != 0 || lp->stride < ((lp->nr + 3) & ~(size_t)3))
        return set_err("%s: a posterior whose columns are %zu floats apart (whole 16-byte pieces of %zu states)", fn, lp->stride, lp->nr);
    return edits_one_of<MapEdits, BAND>(fn, EditsJob{0, 0, lp->nc, seq, seqlen, base, sub, del, ins, low, high}, a, viterbi != 0,
                                        [&](scrappie_hip_engine *e, auto &up) { return (up.post = post_upload_dense(e, fn, lp)) ? 0 : -1; });
}
extern "C" int map_post_edits(const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, int viterbi, float *base,
                              float *sub, float *del, float *ins) {
    return map_edits_one<false>("map_post_edits", lp, stay_pen, skip_pen, local_pen, seq, seqlen, nullptr, nullptr, viterbi, base, sub, del, ins);
}
extern "C" int map_post_edits_banded(const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, const size_t *low,
                                     const size_t *high, int viterbi, float *base, float *sub, float *del, float *ins) {
    return map_edits_one<true>("map_post_edits_banded", lp, stay_pen, skip_pen, local_pen, seq, seqlen, low, high, viterbi, base, sub, del, ins);
}

extern "C" int scrappie_hip_map_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                            const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShMapEditsRead>("map_edits_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}

extern "C" int scrappie_hip_map_edits_banded_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                                   const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShMapEditsBandRead>("map_edits_banded_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}
