/* sh_eng_map_crf_pack.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * one read of a flip-flop (CRF) model against many candidate base sequences (k_map_crf_pack, sh_map_crf_pack.h).
 * scrappie_hip_map_crf_multi_batch: the network and k_crf<true> of a launch group ONCE (run_staged to STOP_POST), every read's candidates packed
 * end to end into workgroups of one k_map_crf_pack launch on the transitions where k_crf left them in d_E, the candidates too long for a pack
 * through k_map_crf (plan_add + dp_run) on the same transitions, scores back; with a path wanted, a second pass of k_map_crf on each read's best
 * candidate alone while d_E still holds the transitions.  scrappie_hip_map_trans_multi: the same on a host matrix and the process-default engine.
 * Both run through sh_eng_cands.inc (the set of a cand array, the launch, the "no admissible path" rule, the launch group, the batch call, the
 * per-read symbol's tail, the form counts); the packing itself is host arithmetic in sh_host.c (scrappie_hip_map_crf_pack_plan).  What is here is
 * the family's own, as a CandTraits: the checks a candidate and a model pass, how a candidate becomes cell words, the pack record's fields, the
 * launch. */

#define SH_MAP_CRF_PACK_CELLS 1024      /* cells a pack holds unless the debug option "map_crf_pack_cells" says otherwise: the fastest on 16 shared candidates of about 150 bases, and faster than k_map_crf per candidate on a call of ~730 bases and 7 edits of it (profiles/map_crf_multi_rate.txt) */

template <> struct CandTraits<ShMapCrfPack> {
    using Rec = ShMapCrfRead;
    static constexpr const char *name = "map_crf_multi";
    static constexpr bool no_path = true;
    static constexpr size_t default_cells = SH_MAP_CRF_PACK_CELLS;
    static PackState &state(scrappie_hip_engine *e) { return e->map_crf_pack; }
    static constexpr auto plan = scrappie_hip_map_crf_pack_plan;
    static std::string why(const char *, const scrappie_hip_map_target &t, size_t, size_t) {
        if (t.seqlen == 0) return "an empty sequence";
        if (t.seqlen > SH_MAP_MAX_SEQ) return "a sequence of " + std::to_string(t.seqlen) + " bases is longer than the " + std::to_string(SH_MAP_MAX_SEQ) + " this build maps";
        const size_t i = first_non_base(t.seq, t.seqlen);
        return i < t.seqlen ? non_base_text(t.seq, i) : std::string();
    }
    /* a candidate of L bases: a cell before its first base and one per base, the last with its place in the pack */
    static void add(CandSet &cs, PackSet::Pack &P, const scrappie_hip_map_target &t) {
        const size_t L = t.seqlen;
        cs.cellw.push_back(SH_MCP_WORD(0, 0, 0, 0, 0));
        for (size_t p = 1; p <= L; p++) cs.cellw.push_back(SH_MCP_WORD(p == L ? P.nitem : 0, p == L, p == 1 ? 1 : 2, t.seq[p - 1], p >= 2 ? t.seq[p - 2] : 0));
        P.ncell += L + 1;
    }
    static size_t lds(const PackSet::Pack &P) { return sh_map_crf_pack_lds_bytes(P.ncell); }
    static size_t read_bytes(size_t L, size_t nblock, bool path) { return map_crf_read_bytes(L, nblock, false, path); }
    static void fill(ShMapCrfPack &q, const CandJob &j, const PackSet::Pack &, size_t) { q.trans = j.at; }
    static int launch(dim3 grid, size_t lds, hipStream_t s, const ShMapCrfArgs &tr, const PackState &d, bool vit, bool tiled) {
        ShMapCrfPackArgs a{};
        a.packs = d.rd.as<ShMapCrfPack>(); a.trans = tr.trans; a.cells = d.cell.as<int>(); a.score = d.score.as<float>();
        return pick_bool([&](auto v, auto tl) {
                using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
                return launch_k<k_map_crf_pack<v(), LD>>(grid, dim3(SH_MAP_NTH), lds, s, a);
            }, vit, tiled);
    }
    static int model_ok(Model *m) {
        return m->arch != 1 ? set_err("map_crf_multi_batch: model '%s' is a transducer model; its candidates are mapped by scrappie_hip_map_multi_batch", m->name.c_str()) : 0;
    }
    static ShMapCrfArgs args(const Model *, const scrappie_hip_params *, const RunOut &ro) {
        ShMapCrfArgs a{};
        a.trans = ro.E;
        return a;
    }
};

extern "C" void scrappie_hip_map_crf_pack_form_counts(uint64_t forms[4]) { cand_form_counts<ShMapCrfPack>(forms); }

extern "C" int scrappie_hip_map_crf_multi_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *cands,
                                                size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_multi_result *out) {
    return cand_batch<ShMapCrfPack>("map_crf_multi_batch", e, model, reads, cands, n, p, viterbi != 0, want_path != 0, out);
}

extern "C" int scrappie_hip_map_trans_multi(const_scrappie_matrix tr, const scrappie_hip_map_target *cand, size_t ncand, int viterbi, float *score) {
    const char *const fn = "map_trans_multi";
    if (!tr || (ncand && (!cand || !score))) return set_err("%s: null argument", fn);
    std::fill(score, score + ncand, NAN);
    if (!sh_crf_post_ok(tr)) return set_err("%s: not a transition matrix of 25 rows and at least one block", fn);
    if (tr->nc > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, tr->nc);
    if (ncand == 0) return 0;
    return cand_one<ShMapCrfPack>(fn, cand, ncand, tr->nr, tr->nc, (int)tr->stride, viterbi != 0, score, ShMapCrfArgs{},
                                  [&](scrappie_hip_engine *e, ShMapCrfArgs &up) { return (up.trans = post_upload_trans(e, fn, tr)) ? 0 : -1; });
}
