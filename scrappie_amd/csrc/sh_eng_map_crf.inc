/* sh_eng_map_crf.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * reads of a flip-flop (CRF) model mapped to base sequences (k_map_crf, sh_map_crf.h).  The per-read symbols map_crf_to_sequence_* on
 * the process-default engine (the caller's host matrix uploaded, the reference-layout loader, one launch), and map_crf_group: what
 * scrappie_hip_map_batch (sh_eng_map.inc) runs for a launch group of such a model -- the network and k_crf<true> (run_staged to
 * STOP_POST), k_map_crf on the transitions where k_crf left them in d_E, k_map_crf_walk; scores and paths back.  Banded and
 * unbanded reads are one kernel and so one plan.  The cutting into launch groups and the two homes are sh_eng_cut.inc's. */

/* host side of one k_map_crf launch, shaped as MapPlan (sh_eng_map.inc) */
struct MapCrfPlan {
    std::vector<ShMapCrfRead> rd;
    std::vector<int> seq, band;
    std::vector<long long> path_off;      /* per read, -1: no path */
    long long tb_words = 0, scr_floats = 0, path_len = 0;
    size_t lds = 0;
};

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

static void map_crf_plan_add(MapCrfPlan &pl, long long trans, int lane, size_t nblock, const int *seq, size_t L, const size_t *lo, const size_t *hi, bool path) {
    ShMapCrfRead r{};
    r.trans = trans; r.lane = lane; r.nblock = (int)nblock; r.seqlen = (int)L; r.ok = 1;
    r.seq = (long long)pl.seq.size();
    pl.seq.insert(pl.seq.end(), seq, seq + L);
    r.band = -1;
    if (lo) {
        r.band = (long long)pl.band.size();
        for (size_t i = 0; i <= nblock; i++) pl.band.push_back((int)lo[i]);
        for (size_t i = 0; i <= nblock; i++) pl.band.push_back((int)hi[i]);
    }
    r.tb = -1;
    if (path) {
        r.tb = pl.tb_words; pl.tb_words += map_crf_tb_words(L, nblock);
        pl.path_off.push_back(pl.path_len); pl.path_len += (long long)nblock + 1;
    } else pl.path_off.push_back(-1);
    if (map_crf_lds_bytes(L) <= SH_MAP_LDS) { r.scr = -1; pl.lds = std::max(pl.lds, map_crf_lds_bytes(L)); }
    else { r.scr = pl.scr_floats; pl.scr_floats += map_crf_scr_floats(L); }
    pl.rd.push_back(r);
}

/* The scratch part of the plan map_crf_plan_add makes of reads of seqlen[i] bases and nblock[i] blocks, in this order in one launch:
 * off[i] = the float offset of read i's four score rows in the scratch allocation, -1 where they live in LDS; returns the floats the
 * launch allocates for them all.  Host arithmetic only, no device: for the tests, which hold it against what k_map_crf touches
 * (4 (L + 2) floats from off[i]). */
extern "C" long long scrappie_hip_map_crf_plan_scratch(const size_t *seqlen, const size_t *nblock, size_t n, long long *off) {
    MapCrfPlan pl;
    std::vector<int> codes;
    for (size_t i = 0; i < n; i++) {
        codes.assign(seqlen[i], 0);
        map_crf_plan_add(pl, 0, 0, nblock[i], codes.data(), seqlen[i], nullptr, nullptr, false);
        if (off) off[i] = pl.rd[i].scr;
    }
    return pl.scr_floats;
}

/* launches of each k_map_crf form in this process: index (vit ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_map_crf_forms[8];
extern "C" void scrappie_hip_map_crf_form_counts(uint64_t forms[8]) {
    if (forms) for (int i = 0; i < 8; i++) forms[i] = g_map_crf_forms[i].load(std::memory_order_relaxed);
}

static const char *const MAP_CRF_NO_PATH = "the sequence has no admissible path through the read (inside its band, where it has one)";

/* one plan through k_map_crf (+ k_map_crf_walk): scores into score[] (NAN where no path is admissible), paths into paths[i] (malloc'd,
 * nblock + 1 entries, only where the plan holds a path and one exists).  trans: d_E or the uploaded matrices.  t[0] += k_map_crf,
 * t[1] += walk + copies. */
static int map_crf_run(scrappie_hip_engine *e, MapCrfPlan &pl, const float *trans, bool vit, bool tiled, float *score, int32_t **paths, double *t) {
    const size_t n = pl.rd.size();
    if (n == 0) return 0;
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_map;
    const bool walk = vit && pl.path_len > 0;
    std::vector<size_t> perm;
    const size_t n_lds = dp_order(pl.rd, perm);
    std::vector<ShMapCrfRead> rd(n);
    std::vector<long long> poff(n);
    for (size_t k = 0; k < n; k++) { rd[k] = pl.rd[perm[k]]; poff[k] = pl.path_off[perm[k]]; }
    if (d.ensure(n, sizeof(ShMapCrfRead), pl.tb_words, pl.scr_floats, pl.path_len) || e->d_map_seq.ensure(pl.seq.size() * 4 + 16) ||
        e->d_map_band.ensure(pl.band.size() * 4 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(d.rd.p, rd.data(), n * sizeof(ShMapCrfRead), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_map_seq.p, pl.seq.data(), pl.seq.size() * 4, hipMemcpyHostToDevice, s));
    if (!pl.band.empty()) HIPCHK(hipMemcpyAsync(e->d_map_band.p, pl.band.data(), pl.band.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.path_off.p, poff.data(), n * 8, hipMemcpyHostToDevice, s));
    ShMapCrfArgs a{};
    a.rd = d.rd.as<ShMapCrfRead>(); a.trans = trans; a.seq = e->d_map_seq.as<int>(); a.band = e->d_map_band.as<int>();
    a.tb = d.tb.as<unsigned>(); a.scr = d.scr.as<float>(); a.score = d.score.as<float>(); a.final_state = d.final_state.as<int>();
    const auto t0 = std::chrono::steady_clock::now();
    if (pick_bool([&](auto v, auto tl) {
            using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
            return dp_launch<k_map_crf<v(), LD, true>, k_map_crf<v(), LD, false>>(s, a, n_lds, n, SH_MAP_NTH, pl.lds, SH_MAPC_HEAD * 4,
                                                                                 g_map_crf_forms + ((v() ? 4 : 0) | (tl() ? 2 : 0)));
        }, vit, tiled)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    const auto t1 = std::chrono::steady_clock::now();
    if (dp_collect<k_map_crf_walk, ShMapCrfRead>(s, d, perm, pl.path_off, pl.path_len, walk, [&](size_t i, float sc, const int32_t *p) {
            const bool none = !(sc >= -SH_MAP_BIG / 2);
            score[i] = none ? NAN : sc;
            if (!paths) return 0;
            paths[i] = nullptr;
            if (!p || none) return 0;
            const size_t ne = (size_t)pl.rd[i].nblock + 1;
            paths[i] = (int32_t *)malloc(ne * 4);
            if (!paths[i]) return set_err("out of host memory");
            memcpy(paths[i], p, ne * 4);
            return 0;
        })) return -1;
    if (t) {
        t[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    return 0;
}

/* the checks every target passes before it reaches the kernel; 0 or -1 with the reason */
static int map_crf_target_ok(const char *fn, size_t nblock, const int *seq, size_t L, const size_t *lo, const size_t *hi, bool band) {
    if (nblock == 0) return set_err("%s: transitions of no blocks", fn);
    if (nblock > (size_t)INT32_MAX / 2) return set_err("%s: %zu blocks is too many", fn, nblock);
    if (L == 0) return set_err("%s: an empty sequence", fn);
    if (L > SH_MAP_MAX_SEQ) return set_err("%s: a sequence of %zu bases is longer than the %d this build maps", fn, L, SH_MAP_MAX_SEQ);
    for (size_t i = 0; i < L; i++)
        if (seq[i] < 0 || seq[i] > 3) return set_err("%s: sequence code %d at %zu is not a base (0..3)", fn, seq[i], i);
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
    map_crf_plan_add(pl, 0, (int)tr->stride, tr->nc, seq, L, band ? lo : nullptr, band ? hi : nullptr, want_path);
    DBuf &dtr = e->d_map_post;
    const size_t nfl = (tr->nc - 1) * tr->stride + 25;           /* as far as the last column's 25th float */
    if (dtr.ensure(nfl * 4)) return NAN;
    if (hipMemcpyAsync(dtr.p, tr->data.f, nfl * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess) { set_err("%s: upload failed", fn); return NAN; }
    float score = NAN;
    int32_t *p = nullptr;
    if (map_crf_run(e, pl, dtr.as<float>(), vit, false, &score, want_path ? &p : nullptr, nullptr)) { (void)hipGetLastError(); return NAN; }
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
/* reads idx[0..cnt) of the call: network + k_crf<true> -> k_map_crf on d_E, on the main stream and under the engine's lock, before
 * anything can overwrite d_E -> k_map_crf_walk */
template <class Cut>
static int map_crf_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const scrappie_hip_map_target *tg, const std::vector<size_t> &idx,
                         const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_result *out, Cut &cut) {
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const raw_table *> win;
    for (size_t r : idx) win.push_back(&reads[r]);
    RunOut ro;
    std::vector<unsigned> bad;
    if (run_staged(e, m, win, p, STOP_POST, 5, &ro, bad, e->map_ms)) return -1;
    const LaunchGroup &lg = e->current().lg;
    MapCrfPlan plan;
    std::vector<size_t> who;
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0) continue;
        const size_t r = idx[(size_t)o];
        if (bad[i]) {
            cut.refuse(r, "the read holds values outside the supported range (is the signal trimmed and med/MAD-normalised?)");
            continue;
        }
        const scrappie_hip_map_target &t = tg[r];
        map_crf_plan_add(plan, lg.tile_boff[i >> 4], (int)(i & 15), (size_t)lg.rT[i], t.seq, t.seqlen, t.poslow, t.poshigh, want_path && vit);
        who.push_back(r);
    }
    const size_t n = who.size();
    if (!n) return 0;
    std::vector<float> sc(n, NAN);
    std::vector<int32_t *> paths(n, nullptr);
    if (map_crf_run(e, plan, ro.E, vit, true, sc.data(), paths.data(), e->map_ms + 1)) {
        for (size_t k = 0; k < n; k++) free(paths[k]);
        return -1;
    }
    for (size_t k = 0; k < n; k++) {
        scrappie_hip_map_result &res = out[who[k]];
        if (std::isnan(sc[k])) { free(paths[k]); cut.refuse(who[k], MAP_CRF_NO_PATH); continue; }
        res.score = sc[k]; res.nblock = (size_t)plan.rd[k].nblock; res.path = paths[k];
    }
    return 0;
}
