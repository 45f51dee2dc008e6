/* sh_eng_map.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * block-based mapping of transducer posteriors to sequences (sh_map.h).  The reference's map_to_sequence_* on the
 * process-default engine (the caller's host posterior uploaded, one launch), and scrappie_hip_map_batch: the network and S1
 * of a launch group (run_staged to STOP_POST), k_map on the posterior where S1 left it, k_map_walk; scores and paths back.
 * A flip-flop (CRF) model takes the same call and the same cut; its launch group is map_crf_group (sh_eng_map_crf.inc).
 * What is here is the family's own: k_map's size formulas and traits, its launch, the checks a target passes, what a read adds to a launch
 * group, map_group.  The cutting of a call into launch groups and dp_launch / dp_collect are sh_eng_cut.inc's; the plan, its runner, the
 * upload of a host posterior, the batch call and the launch group's stage are sh_eng_post.inc's. */

static size_t map_lds_bytes(size_t L) { return (2 * (L + 2) + L) * 4; }
/* the longest sequence whose rows and codes stay in LDS (map_lds_bytes is linear in L) */
extern "C" size_t scrappie_hip_map_lds_max_seq(void) {
    const size_t per = map_lds_bytes(1) - map_lds_bytes(0);
    return (SH_MAP_LDS - map_lds_bytes(0)) / per;
}
/* code words (4 ceil(L / 64) per block) + END bits (one word per 32 blocks), rounded to whole 16-byte pieces */
static long long map_tb_words(size_t L, size_t nblock) {
    return (long long)nblock * (long long)(4 * ((L + 63) / 64)) + (long long)(((nblock + 31) / 32 + 3) & ~(size_t)3);
}
/* device bytes one read adds to a launch (traceback, scratch, path, codes, bands) */
static size_t map_read_bytes(size_t L, size_t nblock, bool band, bool path) {
    size_t b = L * 4 + sizeof(ShMapRead) + 64;
    if (band) b += nblock * 8;
    if (path) b += (size_t)map_tb_words(L, nblock) * 4 + nblock * 4;
    if (map_lds_bytes(L) > SH_MAP_LDS) b += (2 * (L + 2) + 4) * 4;
    return b;
}

/* launches of each k_map form in this process: index (vit ? 8 : 0) | (band ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_map_forms[16];

template <> struct DpTraits<ShMapRead> {
    using Args = ShMapArgs;
    static long long &at(ShMapRead &r) { return r.post; }
    static size_t lds_bytes(size_t L) { return map_lds_bytes(L); }
    static long long scr_floats(size_t L) { return (long long)((2 * (L + 2) + 3) & ~(size_t)3); }
    static long long tb_words(size_t L, size_t nblock) { return map_tb_words(L, nblock); }
    static size_t path_len(size_t nblock) { return nblock; }
    static size_t band_len(size_t nblock) { return nblock; }
    static constexpr auto walk = k_map_walk;
    static bool none(float) { return false; }
    static int launch(hipStream_t s, const ShMapArgs &a, size_t n_lds, size_t n, size_t lds, bool vit, bool band, bool tiled) {
        return pick_bool([&](auto v, auto b, auto tl) {
                return dp_launch<k_map<v(), b(), tl(), true>, k_map<v(), b(), tl(), false>>(s, a, n_lds, n, SH_MAP_NTH, lds, 0,
                                                                                           g_map_forms + ((v() ? 8 : 0) | (b() ? 4 : 0) | (tl() ? 2 : 0)));
            }, vit, band, tiled);
    }
};
/* host side of one k_map launch (DpPlan, sh_eng_post.inc; dp_run takes it through k_map and k_map_walk) */
using MapPlan = DpPlan<ShMapRead>;

/* plan_scratch (sh_eng_post.inc) of k_map's records: for the tests, which hold it against what k_map touches (2 (L + 2) floats from off[i]) */
extern "C" long long scrappie_hip_map_plan_scratch(const size_t *seqlen, const size_t *nblock, size_t n, long long *off) {
    return plan_scratch<ShMapRead>(seqlen, nblock, n, off);
}

/* the checks every target passes before it reaches a kernel; nr: posterior rows; 0 or -1 with the reason */
static int map_target_ok(const char *fn, size_t nr, size_t nblock, const int *seq, size_t L, const size_t *lo, const size_t *hi, bool band) {
    if (nr < 2) return set_err("%s: a posterior of %zu states (at least 2: one k-mer and stay)", fn, nr);
    if (nblock == 0) return set_err("%s: a posterior of no blocks", fn);
    if (nblock > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, nblock);
    if (L == 0) return set_err("%s: an empty sequence", fn);
    if (L > SH_MAP_MAX_SEQ) return set_err("%s: a sequence of %zu states is longer than the %d this build maps", fn, L, SH_MAP_MAX_SEQ);
    for (size_t i = 0; i < L; i++)
        if (seq[i] < 0 || (size_t)seq[i] >= nr - 1) return set_err("%s: sequence state %d at %zu is not one of the posterior's %zu k-mers", fn, seq[i], i, nr - 1);
    if (band) {
        if (L < 3) return set_err("%s: a banded mapping needs a sequence of at least 3 states (got %zu)", fn, L);
        if (!sh_bounds_sane(lo, hi, nblock, L, 0)) return set_err("%s: the bands are not valid (are_bounds_sane)", fn);
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* per-read reference surface (decode.c:1420-1964)                      */
/* ------------------------------------------------------------------ */
static float map_one(const char *fn, const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t L,
                     const size_t *lo, const size_t *hi, bool band, bool vit, int *path) {
    if (!lp || !seq) return NAN;                                       /* RETURN_NULL_IF, decode.c:1423-1424 */
    if (band && (!lo || !hi)) return NAN;
    if (band && L >= 3 && !are_bounds_sane(lo, hi, lp->nc, L)) { set_err("%s: the bands are not valid (are_bounds_sane)", fn); return NAN; }
    if (map_target_ok(fn, lp->nr, lp->nc, seq, L, lo, hi, band)) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    MapPlan pl;
    const bool want_path = vit && !band && path;
    plan_add(pl, 0, 0, lp->nc, seq, L, band ? lo : nullptr, band ? hi : nullptr, want_path);
    ShMapArgs a{};
    a.post = post_upload_dense(e, fn, lp);
    if (!a.post) return NAN;
    a.pstride = (long long)lp->stride; a.nr = (int)lp->nr;
    a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
    float score = NAN;
    int32_t *p = nullptr;
    if (dp_run(e, pl, a, vit, band, false, &score, want_path ? &p : nullptr, nullptr)) { (void)hipGetLastError(); return NAN; }
    if (want_path) {
        if (!p) return NAN;
        memcpy(path, p, lp->nc * 4);
        free(p);
    }
    return score;
}

extern "C" float map_to_sequence_viterbi(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                         int const *seq, size_t seqlen, int *path) {
    return map_one("map_to_sequence_viterbi", logpost, stay_pen, skip_pen, local_pen, seq, seqlen, nullptr, nullptr, false, true, path);
}
extern "C" float map_to_sequence_forward(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                         int const *seq, size_t seqlen) {
    return map_one("map_to_sequence_forward", logpost, stay_pen, skip_pen, local_pen, seq, seqlen, nullptr, nullptr, false, false, nullptr);
}
extern "C" float map_to_sequence_viterbi_banded(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                                int const *seq, size_t seqlen, size_t const *poslow, size_t const *poshigh) {
    return map_one("map_to_sequence_viterbi_banded", logpost, stay_pen, skip_pen, local_pen, seq, seqlen, poslow, poshigh, true, true, nullptr);
}
extern "C" float map_to_sequence_forward_banded(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                                int const *seq, size_t seqlen, size_t const *poslow, size_t const *poshigh) {
    return map_one("map_to_sequence_forward_banded", logpost, stay_pen, skip_pen, local_pen, seq, seqlen, poslow, poshigh, true, false, nullptr);
}

/* ------------------------------------------------------------------ */
/* batched: network + S1 -> k_map -> k_map_walk per launch group        */
/* ------------------------------------------------------------------ */
extern "C" int scrappie_hip_read_blocks(scrappie_hip_engine *e, int model, size_t nsample) {
    Model *m = get_model(e, model);
    if (!m) return -1;
    const size_t ns = m->arch == 3 ? nsample / (size_t)m->nfeat : nsample;
    return (int)std::min<size_t>(map_blocks(m, ns), (size_t)INT32_MAX);
}

extern "C" int scrappie_hip_model_states(scrappie_hip_engine *e, int model) {
    Model *m = get_model(e, model);
    return m ? m->NS : -1;
}

extern "C" void scrappie_hip_map_timing(scrappie_hip_engine *e, double out[3]) { timing3(e ? e->map_ms : nullptr, out); }
extern "C" void scrappie_hip_free_map_results(scrappie_hip_map_result *r, size_t n) { free_paths(r, n); }

/* the posterior of a launch group as k_map and k_map_pack take it */
static ShMapArgs map_group_args(const Model *m, const scrappie_hip_params *p, const RunOut &ro) {
    ShMapArgs a{};
    a.E = ro.E; a.sums = ro.sums; a.nr = m->NS; a.nchunk = m->ff_mtiles; a.min_prob = p->min_prob;
    a.stay_pen = p->stay_pen; a.skip_pen = p->skip_pen; a.local_pen = p->local_pen;
    return a;
}

/* one launch group: reads idx[] of the call (post_group, sh_eng_post.inc), the unbanded through one k_map launch, the banded through another */
static int map_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const scrappie_hip_map_target *tg, const std::vector<size_t> &idx,
                     const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_result *out, LaunchCut<MapLoad> &cut) {
    return post_group(e, m, reads, idx, p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
        MapPlan plan[2];                       /* unbanded, banded */
        std::vector<size_t> who[2];
        for (const PostRead &q : rd) {
            const scrappie_hip_map_target &t = tg[q.r];
            const bool band = t.poslow != nullptr;
            plan_add(plan[band], q.boff, q.lane, q.nblock, t.seq, t.seqlen, t.poslow, t.poshigh, want_path && vit && !band);
            who[band].push_back(q.r);
        }
        const ShMapArgs a = map_group_args(m, p, ro);
        for (int b = 0; b < 2; b++) {
            const size_t n = who[b].size();
            if (!n) continue;
            std::vector<float> sc(n, NAN);
            std::vector<int32_t *> paths(n, nullptr);
            const int rc = dp_run(e, plan[b], a, vit, b == 1, true, sc.data(), paths.data(), e->map_ms + 1);
            for (size_t k = 0; k < n; k++) {
                scrappie_hip_map_result &res = out[who[b][k]];
                if (rc) { free(paths[k]); continue; }
                res.score = sc[k]; res.nblock = (size_t)plan[b].rd[k].nblock; res.path = paths[k];
            }
            if (rc) return -1;
        }
        return 0;
    });
}

extern "C" int scrappie_hip_map_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets,
                                      size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_result *out) {
    PostCall c(e, "map_batch");
    if (c.enter(!n || (reads && targets && out))) return -1;
    bool crf = false;                   /* a flip-flop model: k_map_crf on its transitions (sh_eng_map_crf.inc) */
    if (c.open(model, p, [&](Model *m) {
            crf = m->arch == 1;
            if (crf) return 0;
            int nk = m->NS - 1;             /* NS = 4^k + 1 */
            while (nk > 1 && nk % 4 == 0) nk /= 4;
            return nk != 1 ? set_err("map_batch: model '%s' has %d states, not 4^k + 1", m->name.c_str(), m->NS) : 0;
        })) return -1;
    Model *m = c.m;
    for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].path = nullptr; }
    const bool vit = viterbi != 0, wp = want_path != 0;
    /* launch groups in input order (LaunchCut; PostCall's memory model), each read adding its traceback */
    LaunchCut<MapLoad> cut{e, "map_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) {
        return crf ? map_crf_group(e, m, reads, targets, grp, c.p, vit, wp, out, cut) : map_group(e, m, reads, targets, grp, c.p, vit, wp, out, cut);
    };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        const scrappie_hip_map_target &t = targets[i];
        const size_t T = c.blocks(cut, i, reads[i]);
        if (T == 0) continue;
        const bool band = t.poslow != nullptr || t.poshigh != nullptr;
        if (!t.seq || (crf ? map_crf_target_ok("map_batch", T, t.seq, t.seqlen, t.poslow, t.poshigh, band)
                           : map_target_ok("map_batch", (size_t)m->NS, T, t.seq, t.seqlen, t.poslow, t.poshigh, band)) || (band && !t.poslow)) {
            cut.refuse(i, t.seq ? g_err : "no sequence");
            continue;
        }
        c.add(cut, i, T, crf ? map_crf_read_bytes(t.seqlen, T, band, vit && wp) : map_read_bytes(t.seqlen, T, band, vit && wp && !band),
              "read and sequence too long for one launch group on this device");
    }
    return c.finish(cut, [&] { scrappie_hip_free_map_results(out, n); for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; } });
}
