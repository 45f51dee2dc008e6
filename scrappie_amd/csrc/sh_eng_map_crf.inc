/* sh_eng_map_crf.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * reads of a flip-flop (CRF) model mapped to base sequences (k_map_crf, sh_map_crf.h).  The per-read symbols map_crf_to_sequence_* on
 * the process-default engine (the caller's host matrix uploaded, the reference-layout loader, one launch), and map_crf_group: what
 * scrappie_hip_map_batch (sh_eng_map.inc) runs for a launch group of such a model -- the network and k_crf<true> (run_staged to
 * STOP_POST), k_map_crf on the transitions where k_crf left them in d_E, k_map_crf_walk; scores and paths back.  Banded and
 * unbanded reads are one kernel and so one plan.  What is here is the family's own: k_map_crf's size formulas and traits, its launch, the
 * "no admissible path" rule, the checks a target passes.  The cutting into launch groups and dp_launch / dp_collect are sh_eng_cut.inc's; the
 * plan, its runner, the upload of a host matrix and the launch group's stage are sh_eng_post.inc's. */

/* two columns of transitions, two buffers of a B row and an S row (cells 0 .. L and the spare slot), the codes */
static size_t map_crf_lds_bytes(size_t L) { return (SH_MAPC_HEAD + 4 * (L + 2) + L) * 4; }
/* the longest sequence whose rows and codes stay in LDS (map_crf_lds_bytes is linear in L) */
extern "C" size_t scrappie_hip_map_crf_lds_max_seq(void) {
    const size_t per = map_crf_lds_bytes(1) - map_crf_lds_bytes(0);
    return (SH_MAP_LDS - map_crf_lds_bytes(0)) / per;
}
static long long map_crf_scr_floats(size_t L) { return (long long)(4 * (L + 2)); }       /* a multiple of 4: starts stay 16-byte aligned */
/* 4 ceil((L + 1) / 64) words per block: whole 16-byte pieces */
static long long map_crf_tb_words(size_t L, size_t nblock) { return (long long)nblock * (long long)(4 * ((L + 64) / 64)); }
/* device bytes one read adds to a launch (traceback, scratch, path, codes, bands) */
static size_t map_crf_read_bytes(size_t L, size_t nblock, bool band, bool path) {
    size_t b = L * 4 + sizeof(ShMapCrfRead) + 64;
    if (band) b += (nblock + 1) * 8;
    if (path) b += (size_t)map_crf_tb_words(L, nblock) * 4 + (nblock + 1) * 4;
    if (map_crf_lds_bytes(L) > SH_MAP_LDS) b += (size_t)map_crf_scr_floats(L) * 4;
    return b;
}

/* launches of each k_map_crf form in this process: index (vit ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_map_crf_forms[8];
extern "C" void scrappie_hip_map_crf_form_counts(uint64_t forms[8]) {
    if (forms) for (int i = 0; i < 8; i++) forms[i] = g_map_crf_forms[i].load(std::memory_order_relaxed);
}

static const char *const MAP_CRF_NO_PATH = "the sequence has no admissible path through the read (inside its band, where it has one)";

template <> struct DpTraits<ShMapCrfRead> {
    using Args = ShMapCrfArgs;
    static long long &at(ShMapCrfRead &r) { return r.trans; }
    static size_t lds_bytes(size_t L) { return map_crf_lds_bytes(L); }
    static long long scr_floats(size_t L) { return map_crf_scr_floats(L); }
    static long long tb_words(size_t L, size_t nblock) { return map_crf_tb_words(L, nblock); }
    static size_t path_len(size_t nblock) { return nblock + 1; }
    static size_t band_len(size_t nblock) { return nblock + 1; }
    static constexpr auto walk = k_map_crf_walk;
    static bool none(float sc) { return !(sc >= -SH_MAP_BIG / 2); }
    /* (banded and unbanded reads are one kernel: its callers pass band = false) */
    static int launch(hipStream_t s, const ShMapCrfArgs &a, size_t n_lds, size_t n, size_t lds, bool vit, bool, bool tiled) {
        return pick_bool([&](auto v, auto tl) {
                using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
                return dp_launch<k_map_crf<v(), LD, true>, k_map_crf<v(), LD, false>>(s, a, n_lds, n, SH_MAP_NTH, lds, SH_MAPC_HEAD * 4,
                                                                                     g_map_crf_forms + ((v() ? 4 : 0) | (tl() ? 2 : 0)));
            }, vit, tiled);
    }
};
/* host side of one k_map_crf launch (DpPlan, sh_eng_post.inc; dp_run takes it through k_map_crf and k_map_crf_walk: scores NAN where no path is
 * admissible, paths of nblock + 1 entries) */
using MapCrfPlan = DpPlan<ShMapCrfRead>;

/* plan_scratch (sh_eng_post.inc) of k_map_crf's records: for the tests, which hold it against what k_map_crf touches (4 (L + 2) floats from off[i]) */
extern "C" long long scrappie_hip_map_crf_plan_scratch(const size_t *seqlen, const size_t *nblock, size_t n, long long *off) {
    return plan_scratch<ShMapCrfRead>(seqlen, nblock, n, off);
}

/* the checks every target passes before it reaches the kernel; 0 or -1 with the reason */
static int map_crf_target_ok(const char *fn, size_t nblock, const int *seq, size_t L, const size_t *lo, const size_t *hi, bool band) {
    if (nblock == 0) return set_err("%s: transitions of no blocks", fn);
    if (nblock > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, nblock);
    if (L == 0) return set_err("%s: an empty sequence", fn);
    if (L > SH_MAP_MAX_SEQ) return set_err("%s: a sequence of %zu bases is longer than the %d this build maps", fn, L, SH_MAP_MAX_SEQ);
    if (bases_ok(fn, seq, L)) return -1;
    if (band && !scrappie_hip_map_crf_bounds_sane(lo, hi, nblock, L)) return set_err("%s: the bands are not valid (scrappie_hip_map_crf_bounds_sane)", fn);
    return 0;
}

/* ------------------------------------------------------------------ */
/* per-read symbols                                                     */
/* ------------------------------------------------------------------ */
static float map_crf_one(const char *fn, const_scrappie_matrix tr, const int *seq, size_t L, const size_t *lo, const size_t *hi, bool band, bool vit, int *path) {
    if (!tr || !seq || (band && (!lo || !hi))) { set_err("%s: null argument", fn); return NAN; }
    if (!sh_crf_post_ok(tr)) { set_err("%s: not a transition matrix of 25 rows and at least one block", fn); return NAN; }
    if (map_crf_target_ok(fn, tr->nc, seq, L, lo, hi, band)) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    MapCrfPlan pl;
    const bool want_path = vit && path;
    plan_add(pl, 0, (int)tr->stride, tr->nc, seq, L, band ? lo : nullptr, band ? hi : nullptr, want_path);
    const float *dtr = post_upload_trans(e, fn, tr);
    if (!dtr) return NAN;
    float score = NAN;
    int32_t *p = nullptr;
    ShMapCrfArgs a{};
    a.trans = dtr;
    if (dp_run(e, pl, a, vit, false, false, &score, want_path ? &p : nullptr, nullptr)) { (void)hipGetLastError(); return NAN; }
    if (std::isnan(score)) { free(p); set_err("%s: %s", fn, MAP_CRF_NO_PATH); return NAN; }
    if (want_path) {
        if (!p) return NAN;
        memcpy(path, p, (tr->nc + 1) * 4);
        free(p);
    }
    return score;
}

extern "C" float map_crf_to_sequence_viterbi(const_scrappie_matrix trans, int const *seq, size_t seqlen, int *path) {
    return map_crf_one("map_crf_to_sequence_viterbi", trans, seq, seqlen, nullptr, nullptr, false, true, path);
}
extern "C" float map_crf_to_sequence_forward(const_scrappie_matrix trans, int const *seq, size_t seqlen) {
    return map_crf_one("map_crf_to_sequence_forward", trans, seq, seqlen, nullptr, nullptr, false, false, nullptr);
}
extern "C" float map_crf_to_sequence_viterbi_banded(const_scrappie_matrix trans, int const *seq, size_t seqlen, size_t const *low, size_t const *high, int *path) {
    return map_crf_one("map_crf_to_sequence_viterbi_banded", trans, seq, seqlen, low, high, true, true, path);
}
extern "C" float map_crf_to_sequence_forward_banded(const_scrappie_matrix trans, int const *seq, size_t seqlen, size_t const *low, size_t const *high) {
    return map_crf_one("map_crf_to_sequence_forward_banded", trans, seq, seqlen, low, high, true, false, nullptr);
}

/* ------------------------------------------------------------------ */
/* batched: one launch group of scrappie_hip_map_batch                  */
/* ------------------------------------------------------------------ */
/* reads idx[] of the call (post_group, sh_eng_post.inc): k_map_crf on d_E -> k_map_crf_walk */
template <class Cut>
static int map_crf_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const scrappie_hip_map_target *tg, const std::vector<size_t> &idx,
                         const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_result *out, Cut &cut) {
    return post_group(e, m, reads, idx, p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
        const size_t n = rd.size();
        if (!n) return 0;
        MapCrfPlan plan;
        for (const PostRead &q : rd) plan_add(plan, q.boff, q.lane, q.nblock, tg[q.r].seq, tg[q.r].seqlen, tg[q.r].poslow, tg[q.r].poshigh, want_path && vit);
        std::vector<float> sc(n, NAN);
        std::vector<int32_t *> paths(n, nullptr);
        ShMapCrfArgs a{};
        a.trans = ro.E;
        if (dp_run(e, plan, a, vit, false, true, sc.data(), paths.data(), e->map_ms + 1)) {
            for (size_t k = 0; k < n; k++) free(paths[k]);
            return -1;
        }
        for (size_t k = 0; k < n; k++) {
            scrappie_hip_map_result &res = out[rd[k].r];
            if (std::isnan(sc[k])) { free(paths[k]); cut.refuse(rd[k].r, MAP_CRF_NO_PATH); continue; }
            res.score = sc[k]; res.nblock = rd[k].nblock; res.path = paths[k];
        }
        return 0;
    });
}
