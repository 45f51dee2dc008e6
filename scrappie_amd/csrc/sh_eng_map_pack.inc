/* sh_eng_map_pack.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * one read against many candidate sequences (k_map_pack, sh_map_pack.h).  scrappie_hip_map_multi_batch: the network and S1 of a
 * launch group ONCE (run_staged to STOP_POST, as map_group), every read's candidates packed end to end into workgroups of one
 * k_map_pack launch on the posterior where S1 left it, the candidates too long for a pack through k_map (plan_add + dp_run) on
 * the same posterior, scores back; with a path wanted, a second pass of k_map on each read's best candidate alone while the
 * posterior is still resident.  scrappie_hip_map_post_multi: the same on a host posterior and the process-default engine.
 * Both run through sh_eng_cands.inc (the set of a cand array, the launch, the launch group, the batch call, the per-read symbol's tail, the form
 * counts); the packing itself is host arithmetic in sh_host.c (scrappie_hip_map_pack_plan).  What is here is the family's own, as a CandTraits: the
 * checks a candidate and a model pass, how a candidate becomes cell words and first cells, the pack record's fields, the launch. */

#define SH_MAP_PACK_CELLS 256       /* cells a pack holds unless the debug option "map_pack_cells" says otherwise: the fastest on 24 barcodes of 40 bases, faster than k_map per candidate on 8 x 400 bases (profiles/map_multi_rate.txt) */

/* the state codes share a cell word with the cell's kind */
static int map_pack_states_ok(const char *fn, size_t nr) {
    return nr > (size_t)SH_MPK_CODE_MASK ? set_err("%s: a posterior of %zu states is more than a pack's cell words hold", fn, nr) : 0;
}

template <> struct CandTraits<ShMapPack> {
    using Rec = ShMapRead;
    static constexpr const char *name = "map_multi";
    static constexpr bool no_path = false;                   /* k_map's score as it is */
    static constexpr size_t default_cells = SH_MAP_PACK_CELLS;
    static PackState &state(scrappie_hip_engine *e) { return e->map_pack; }
    static constexpr auto plan = scrappie_hip_map_pack_plan;
    static std::string why(const char *fn, const scrappie_hip_map_target &t, size_t nr, size_t nblock) {
        if (!map_target_ok(fn, nr, nblock, t.seq, t.seqlen, nullptr, nullptr, false)) return std::string();
        const std::string pre = std::string(fn) + ": ";      /* (map_target_ok's texts begin with fn, as the caller's own will) */
        return strncmp(g_err, pre.c_str(), pre.size()) ? g_err : g_err + pre.size();
    }
    /* a candidate of L states: a start cell, its states, an end cell; a pack's first cells: each candidate's and the pack's end */
    static void add(CandSet &cs, PackSet::Pack &P, const scrappie_hip_map_target &t) {
        if (P.nitem == 0) cs.firsts.push_back(0);
        cs.cellw.push_back(SH_MPK_START << SH_MPK_KIND_SHIFT);
        for (size_t i = 0; i < t.seqlen; i++) cs.cellw.push_back(((i == 0 ? SH_MPK_POS0 : i == 1 ? SH_MPK_POS1 : SH_MPK_POS2) << SH_MPK_KIND_SHIFT) | t.seq[i]);
        cs.cellw.push_back(SH_MPK_END << SH_MPK_KIND_SHIFT);
        P.ncell += t.seqlen + 2;
        cs.firsts.push_back((int)P.ncell);
    }
    static size_t lds(const PackSet::Pack &P) { return sh_map_pack_lds_bytes(P.ncell, P.nitem); }
    static size_t read_bytes(size_t L, size_t nblock, bool path) { return map_read_bytes(L, nblock, false, path); }
    static void fill(ShMapPack &q, const CandJob &j, const PackSet::Pack &P, size_t first) { q.post = j.at; q.first = (long long)first; q.ncand = (int)P.nitem; }
    static int launch(dim3 grid, size_t lds, hipStream_t s, ShMapArgs a, const PackState &d, bool vit, bool tiled) {
        a.score = d.score.as<float>();
        return pick_bool([&](auto v, auto tl) {
                return launch_k<k_map_pack<v(), tl()>>(grid, dim3(SH_MAP_NTH), lds, s, a, (const ShMapPack *)d.rd.p, (const int *)d.cell.p, (const int *)d.first.p);
            }, vit, tiled);
    }
    static int model_ok(Model *m) {
        if (m->arch == 1) return set_err("map_multi_batch: model '%s' is a flip-flop (CRF) model; candidates are mapped with transducer models only", m->name.c_str());
        int nk = m->NS - 1;
        while (nk > 1 && nk % 4 == 0) nk /= 4;
        if (nk != 1) return set_err("map_multi_batch: model '%s' has %d states, not 4^k + 1", m->name.c_str(), m->NS);
        return map_pack_states_ok("map_multi_batch", (size_t)m->NS);
    }
    static ShMapArgs args(const Model *m, const scrappie_hip_params *p, const RunOut &ro) { return map_group_args(m, p, ro); }
};

extern "C" void scrappie_hip_map_pack_form_counts(uint64_t forms[4]) { cand_form_counts<ShMapPack>(forms); }

extern "C" int scrappie_hip_map_multi_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *cands,
                                            size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_multi_result *out) {
    return cand_batch<ShMapPack>("map_multi_batch", e, model, reads, cands, n, p, viterbi != 0, want_path != 0, out);
}

extern "C" int scrappie_hip_map_post_multi(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                           const scrappie_hip_map_target *cand, size_t ncand, int viterbi, float *score) {
    const char *const fn = "map_post_multi";
    if (!logpost || (ncand && (!cand || !score))) return set_err("%s: null argument", fn);
    std::fill(score, score + ncand, NAN);
    if (ncand == 0) return 0;
    if (map_pack_states_ok(fn, logpost->nr)) return -1;
    ShMapArgs a{};
    a.pstride = (long long)logpost->stride; a.nr = (int)logpost->nr;
    a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
    return cand_one<ShMapPack>(fn, cand, ncand, logpost->nr, logpost->nc, 0, viterbi != 0, score, a,
                               [&](scrappie_hip_engine *e, ShMapArgs &up) { return (up.post = post_upload_dense(e, fn, logpost)) ? 0 : -1; });
}
