/* sh_eng_map_edits.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * every single-base edit of a sequence scored against a read of a transducer model (k_map_edits_rows, k_map_edits, sh_map_edits.h).
 * scrappie_hip_map_edits_batch: the network and S1 of a launch group once, then the three kernels on the posterior where S1 left it in d_E;
 * map_post_edits: the same on a host posterior and the process-default engine.  Both run through sh_eng_edits.inc; the debug option
 * "map_edits_budget_kb" cuts a launch group's reads into several launches.  What is here is the family's own, as an EditsTraits: the checks a
 * target and a model pass, the k-mer states of a read's bases, the record's fields, the LDS of its kernels and their forms.  The layout of a
 * launch's buffers is scrappie_hip_map_edits_plan's (sh_host.c). */

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

extern "C" void scrappie_hip_map_edits_form_counts(uint64_t forms[12]) { edits_form_counts<ShMapEditsRead>(forms); }
extern "C" void scrappie_hip_map_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes) {
    if (e) edits_timing(e->map_edits, ms, launches, row_bytes);
}

extern "C" int map_post_edits(const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, int viterbi, float *base,
                              float *sub, float *del, float *ins) {
    const char *const fn = "map_post_edits";
    edits_nan(seq, seqlen, base, sub, del, ins);
    if (!lp || (!seq && seqlen)) return set_err("%s: null argument", fn);
    ShMapEditsArgs a{};
    a.pstride = (long long)lp->stride; a.nr = (int)lp->nr; a.k = map_edits_kmer(lp->nr);
    a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
    if (!a.k) return set_err("%s: a posterior of %zu rows is not 4^k + 1 states for k = 1 .. %d", fn, lp->nr, SH_ME_K);
    if (lp->nc == 0) return set_err("%s: a posterior of no blocks", fn);
    if (lp->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, lp->nc);
    if (lp->stride % 4 != 0 || lp->stride < ((lp->nr + 3) & ~(size_t)3))
        return set_err("%s: a posterior whose columns are %zu floats apart (whole 16-byte pieces of %zu states)", fn, lp->stride, lp->nr);
    const std::string why = EditsTraits<ShMapEditsRead>::target_why(scrappie_hip_map_target{seq, seqlen, nullptr, nullptr}, a);
    if (!why.empty()) { set_err("%s: %s", fn, why.c_str()); return 0; }      /* every score NAN, the reason as the error text */
    return edits_one<ShMapEditsRead>(EditsJob{0, 0, lp->nc, seq, seqlen, base, sub, del, ins}, a, viterbi != 0,
                                     [&](scrappie_hip_engine *e, ShMapEditsArgs &up) { return (up.post = post_upload_dense(e, fn, lp)) ? 0 : -1; });
}

extern "C" int scrappie_hip_map_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                            const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out) {
    return edits_batch<ShMapEditsRead>("map_edits_batch", e, model, reads, targets, n, p, viterbi != 0, out);
}
