/* sh_eng_map.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * block-based mapping of transducer posteriors to sequences (sh_map.h).  The reference's map_to_sequence_* on the
 * process-default engine (the caller's host posterior uploaded, one launch), and scrappie_hip_map_batch: the network and S1
 * of a launch group (run_staged to STOP_POST), k_map on the posterior where S1 left it, k_map_walk; scores and paths back.
 * A flip-flop (CRF) model takes the same call and the same cut; its launch group is map_crf_group (sh_eng_map_crf.inc).
 * What is here is the family's own: the plan of a launch, the checks a target passes, the cost of a launch group, map_group.
 * The cutting of a call into launch groups and the run of the records through k_map's two homes are sh_eng_cut.inc's. */

/* host side of one k_map launch: the reads' tables, their codes and bands laid end to end, traceback / scratch offsets */
struct MapPlan {
    std::vector<ShMapRead> rd;
    std::vector<int> seq, band;
    std::vector<long long> path_off;      /* per read, -1: no path */
    long long tb_words = 0, scr_floats = 0, path_len = 0;
    size_t lds = 0;
};

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

static void plan_add(MapPlan &pl, long long post, int lane, size_t nblock, const int *seq, size_t L, const size_t *lo, const size_t *hi, bool path) {
    ShMapRead r{};
    r.post = post; r.lane = lane; r.nblock = (int)nblock; r.seqlen = (int)L; r.ok = 1;
    r.seq = (long long)pl.seq.size();
    pl.seq.insert(pl.seq.end(), seq, seq + L);
    r.band = -1;
    if (lo) {
        r.band = (long long)pl.band.size();
        for (size_t i = 0; i < nblock; i++) pl.band.push_back((int)lo[i]);
        for (size_t i = 0; i < nblock; i++) pl.band.push_back((int)hi[i]);
    }
    r.tb = -1;
    if (path) {
        r.tb = pl.tb_words; pl.tb_words += map_tb_words(L, nblock);
        pl.path_off.push_back(pl.path_len); pl.path_len += (long long)nblock;
    } else pl.path_off.push_back(-1);
    if (map_lds_bytes(L) <= SH_MAP_LDS) { r.scr = -1; pl.lds = std::max(pl.lds, map_lds_bytes(L)); }
    else { r.scr = pl.scr_floats; pl.scr_floats += (long long)((2 * (L + 2) + 3) & ~(size_t)3); }
    pl.rd.push_back(r);
}

/* The scratch part of the plan plan_add makes of reads of seqlen[i] states and nblock[i] blocks, in this order in one launch
 * (no traceback, no bands): off[i] = the float offset of read i's two score rows in the scratch allocation, -1 where they live
 * in LDS; returns the floats the launch allocates for them all.  Host arithmetic only, no device: for the tests, which hold
 * it against what k_map touches (2 (L + 2) floats from off[i]). */
extern "C" long long scrappie_hip_map_plan_scratch(const size_t *seqlen, const size_t *nblock, size_t n, long long *off) {
    MapPlan pl;
    std::vector<int> codes;
    for (size_t i = 0; i < n; i++) {
        codes.assign(seqlen[i], 0);
        plan_add(pl, 0, 0, nblock[i], codes.data(), seqlen[i], nullptr, nullptr, false);
        if (off) off[i] = pl.rd[i].scr;
    }
    return pl.scr_floats;
}

/* launches of each k_map form in this process: index (vit ? 8 : 0) | (band ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_map_forms[16];

/* one plan (all banded or all unbanded) through k_map (+ k_map_walk): scores into score[], paths into paths[i] (malloc'd,
 * only where the plan holds a path).  a: the posterior, its shape and the penalties.  t[0] += k_map, t[1] += walk + copies. */
static int map_run(scrappie_hip_engine *e, MapPlan &pl, ShMapArgs a, bool vit, bool band, bool tiled, float *score, int32_t **paths, double *t) {
    const size_t n = pl.rd.size();
    if (n == 0) return 0;
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_map;
    const bool walk = vit && !band && pl.path_len > 0;
    std::vector<size_t> perm;
    const size_t n_lds = dp_order(pl.rd, perm);
    std::vector<ShMapRead> rd(n);
    std::vector<long long> poff(n);
    for (size_t k = 0; k < n; k++) { rd[k] = pl.rd[perm[k]]; poff[k] = pl.path_off[perm[k]]; }
    if (d.ensure(n, sizeof(ShMapRead), pl.tb_words, pl.scr_floats, pl.path_len) || e->d_map_seq.ensure(pl.seq.size() * 4 + 16) ||
        e->d_map_band.ensure(pl.band.size() * 4 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(d.rd.p, rd.data(), n * sizeof(ShMapRead), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_map_seq.p, pl.seq.data(), pl.seq.size() * 4, hipMemcpyHostToDevice, s));
    if (!pl.band.empty()) HIPCHK(hipMemcpyAsync(e->d_map_band.p, pl.band.data(), pl.band.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.path_off.p, poff.data(), n * 8, hipMemcpyHostToDevice, s));
    a.rd = d.rd.as<ShMapRead>(); a.seq = e->d_map_seq.as<int>(); a.band = e->d_map_band.as<int>(); a.tb = d.tb.as<unsigned>(); a.scr = d.scr.as<float>();
    a.score = d.score.as<float>(); a.final_state = d.final_state.as<int>();
    const auto t0 = std::chrono::steady_clock::now();
    if (pick_bool([&](auto v, auto b, auto t) {
            return dp_launch<k_map<v(), b(), t(), true>, k_map<v(), b(), t(), false>>(s, a, n_lds, n, SH_MAP_NTH, pl.lds, 0,
                                                                                     g_map_forms + ((v() ? 8 : 0) | (b() ? 4 : 0) | (t() ? 2 : 0)));
        }, vit, band, tiled)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    const auto t1 = std::chrono::steady_clock::now();
    if (dp_collect<k_map_walk, ShMapRead>(s, d, perm, pl.path_off, pl.path_len, walk, [&](size_t i, float sc, const int32_t *p) {
            score[i] = sc;
            if (!paths) return 0;
            paths[i] = nullptr;
            if (!p) return 0;
            const size_t nb = (size_t)pl.rd[i].nblock;
            paths[i] = (int32_t *)malloc(nb * 4);
            if (!paths[i]) return set_err("out of host memory");
            memcpy(paths[i], p, nb * 4);
            return 0;
        })) return -1;
    if (t) {
        t[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    return 0;
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
    DBuf &dpost = e->d_map_post;
    const size_t pbytes = lp->nc * lp->stride * 4;
    if (dpost.ensure(pbytes)) return NAN;
    if (hipMemcpyAsync(dpost.p, lp->data.f, pbytes, hipMemcpyHostToDevice, e->stream) != hipSuccess) { set_err("%s: upload failed", fn); return NAN; }
    ShMapArgs a{};
    a.post = dpost.as<float>(); a.pstride = (long long)lp->stride; a.nr = (int)lp->nr;
    a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
    float score = NAN;
    int32_t *p = nullptr;
    if (map_run(e, pl, a, vit, band, false, &score, want_path ? &p : nullptr, nullptr)) { (void)hipGetLastError(); return NAN; }
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
static size_t map_read_nsample(const Model *m, const raw_table &rt) {
    const size_t nf = (rt.raw && rt.end > rt.start) ? rt.end - rt.start : 0;
    return m->arch == 3 ? nf / (size_t)m->nfeat : nf;            /* events: raw holds [nevent][12] features */
}
static size_t map_blocks(const Model *m, size_t ns) {
    return ns >= m->min_samples ? (ns + (size_t)m->stride - 1) / (size_t)m->stride : 0;       /* build_group */
}

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

/* what a launch group holds so far, as its cost counts it */
struct MapLoad { size_t sumT = 0, maxT = 0, extra = 0; };

/* one launch group: reads idx[0..cnt) of the call */
static int map_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const scrappie_hip_map_target *tg, const std::vector<size_t> &idx,
                     const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_result *out, LaunchCut<MapLoad> &cut) {
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const raw_table *> win;
    for (size_t r : idx) win.push_back(&reads[r]);
    RunOut ro;
    std::vector<unsigned> bad;
    if (run_staged(e, m, win, p, STOP_POST, 5, &ro, bad, e->map_ms)) return -1;
    const LaunchGroup &lg = e->current().lg;
    MapPlan plan[2];                       /* unbanded, banded */
    std::vector<size_t> who[2];
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0) continue;
        const size_t r = idx[(size_t)o];
        if (bad[i]) {
            cut.refuse(r, "the read holds values outside the supported range (is the signal trimmed and med/MAD-normalised?)");
            continue;
        }
        const scrappie_hip_map_target &t = tg[r];
        const bool band = t.poslow != nullptr;
        plan_add(plan[band], lg.tile_boff[i >> 4], (int)(i & 15), (size_t)lg.rT[i], t.seq, t.seqlen, t.poslow, t.poshigh, want_path && vit && !band);
        who[band].push_back(r);
    }
    ShMapArgs a{};
    a.E = ro.E; a.sums = ro.sums; a.nr = m->NS; a.nchunk = m->ff_mtiles; a.min_prob = p->min_prob;
    a.stay_pen = p->stay_pen; a.skip_pen = p->skip_pen; a.local_pen = p->local_pen;
    for (int b = 0; b < 2; b++) {
        const size_t n = who[b].size();
        if (!n) continue;
        std::vector<float> sc(n, NAN);
        std::vector<int32_t *> paths(n, nullptr);
        const int rc = map_run(e, plan[b], a, vit, b == 1, true, sc.data(), paths.data(), e->map_ms + 1);
        for (size_t k = 0; k < n; k++) {
            scrappie_hip_map_result &res = out[who[b][k]];
            if (rc) { free(paths[k]); continue; }
            res.score = sc[k]; res.nblock = (size_t)plan[b].rd[k].nblock; res.path = paths[k];
        }
        if (rc) return -1;
    }
    return 0;
}

extern "C" int scrappie_hip_map_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets,
                                      size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_result *out) {
    if (!e || (n && (!reads || !targets || !out))) return set_err("map_batch: null argument");
    std::lock_guard<std::mutex> call(e->call_mu);
    Model *m = get_model(e, model);
    if (!m) return -1;
    const bool crf = m->arch == 1;      /* a flip-flop model: k_map_crf on its transitions (sh_eng_map_crf.inc) */
    if (!crf) {   /* NS = 4^k + 1 */
        int nk = m->NS - 1;
        while (nk > 1 && nk % 4 == 0) nk /= 4;
        if (nk != 1) return set_err("map_batch: model '%s' has %d states, not 4^k + 1", m->name.c_str(), m->NS);
    }
    scrappie_hip_params dp = scrappie_hip_default_params();
    if (!p) p = &dp;
    (void)hipSetDevice(e->device);
    for (double &x : e->map_ms) x = 0.0;
    for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].path = nullptr; }
    const bool vit = viterbi != 0, wp = want_path != 0;
    /* launch groups in input order (LaunchCut), bounded by reads and by device memory: the materialised posterior and the arena of the network
     * (bytes_per_block with the posterior: ~66 KB per column block of 16 reads for 4^5 + 1 states), plus each read's traceback */
    const size_t bpb = bytes_per_block(m, true);
    const size_t budget = e->max_launch_blocks ? e->max_launch_blocks * bpb : (size_t)(e->mem_frac * (double)e->total_mem);
    auto cost = [&](size_t sT, size_t mT, size_t ex) { return (sT / 16 + mT + 1) * bpb + ex; };
    LaunchCut<MapLoad> cut{e, "map_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLoad &) {
        return crf ? map_crf_group(e, m, reads, targets, grp, p, vit, wp, out, cut) : map_group(e, m, reads, targets, grp, p, vit, wp, out, cut);
    };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        const scrappie_hip_map_target &t = targets[i];
        const size_t T = map_blocks(m, map_read_nsample(m, reads[i]));
        if (T == 0) { cut.refuse(i, "read too short for the model (or empty)"); continue; }
        const bool band = t.poslow != nullptr || t.poshigh != nullptr;
        if (!t.seq || (crf ? map_crf_target_ok("map_batch", T, t.seq, t.seqlen, t.poslow, t.poshigh, band)
                           : map_target_ok("map_batch", (size_t)m->NS, T, t.seq, t.seqlen, t.poslow, t.poshigh, band)) || (band && !t.poslow)) {
            cut.refuse(i, t.seq ? g_err : "no sequence");
            continue;
        }
        const size_t rb = crf ? map_crf_read_bytes(t.seqlen, T, band, vit && wp) : map_read_bytes(t.seqlen, T, band, vit && wp && !band);
        if (cost(T, T, rb) > budget) { cut.refuse(i, "read and sequence too long for one launch group on this device"); continue; }
        MapLoad &g = cut.load;
        cut.add(i, cut.who.size() < e->max_launch_reads && cost(g.sumT + T, std::max(g.maxT, T), g.extra + rb) <= budget);
        g.sumT += T; g.maxT = std::max(g.maxT, T); g.extra += rb;
    }
    return cut.finish([&] { scrappie_hip_free_map_results(out, n); for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; } },
                      [](size_t i, const char *why) { set_err("map_batch: read %zu: %s", i, why); });
}
