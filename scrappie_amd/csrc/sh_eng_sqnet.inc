/* sh_eng_sqnet.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * prediction of squiggles from base sequences (sh_sqnet.h).  scrappie_hip_squiggle_predict_batch lays the accepted sequences of a
 * call end to end and cuts them into launches that fit a share of the free device memory (LaunchCut, sh_eng_cut.inc: here are only the checks a
 * sequence passes, what it costs and how a launch is run); a launch is one upload (tiles + codes)
 * -> k_sqnet over all tiles -> one download (3 floats per position) -> transform_units on the host (libm expf, the reference's
 * expressions).  The reference's squiggle_r94 / squiggle_r94_rna / squiggle_r10 are a batch of one on the process-default engine,
 * their model found by name (scrappie_hip_register_model / SCRAPPIE_MODEL_DIR: weights are data here). */

/* .scrm matrices (scrappie_amd/model.py: arch 'squiggle') -> the weight table of k_sqnet */
static int sqnet_load(Model *m, const std::vector<std::pair<std::string, HostMat>> &mats) {
    const char *name = m->name.c_str();
    const HostMat *em = find_mat(mats, "embed_W");
    const HostMat *cw[6], *cb[6];
    for (int l = 0; l < 6; l++) {
        char nm[32];
        snprintf(nm, sizeof nm, "conv%d_W", l + 1); cw[l] = find_mat(mats, nm);
        snprintf(nm, sizeof nm, "conv%d_b", l + 1); cb[l] = find_mat(mats, nm);
        if (!cw[l] || !cb[l]) return set_err("model '%s': missing %s or its bias", name, nm);
    }
    if (!em) return set_err("model '%s': missing embed_W", name);
    if (em->nr != SH_SQN_NE || em->nc != 4) return set_err("model '%s': embed_W is %d x %d, this build runs 4 bases -> %d features", name, em->nc, em->nr, SH_SQN_NE);
    if (m->stride != 1 || m->conv_act != 1) return set_err("model '%s': a squiggle model has stride 1 and tanh", name);
    const int WL = cw[0]->nr / SH_SQN_NE;
    if ((WL != 7 && WL != 9) || cw[0]->nr != WL * SH_SQN_NE)
        return set_err("model '%s': conv1_W has %d rows: this build runs windows of 7 and 9 over %d features", name, cw[0]->nr, SH_SQN_NE);
    for (int l = 0; l < 6; l++) {
        const int cin = l == 0 ? SH_SQN_NE : SH_SQN_NF, cout = l == 5 ? SH_SQN_NO : SH_SQN_NF;
        if (cw[l]->nr != WL * cin || cw[l]->nc != cout || cb[l]->nr * cb[l]->nc != cout)
            return set_err("model '%s': conv%d is %d x %d with a bias of %d: this build runs %d -> %d filters over a window of %d", name, l + 1, cw[l]->nc, cw[l]->nr,
                           cb[l]->nr * cb[l]->nc, cin, cout, WL);
    }
    for (auto &kv : mats) for (float x : kv.second.v) if (!std::isfinite(x)) return set_err("model '%s': %s holds a non-finite weight", name, kv.first.c_str());
    std::vector<float> t((size_t)sqn_table_floats(WL), 0.0f);
    for (int c = 0; c < 4; c++) for (int r = 0; r < SH_SQN_NE; r++) t[(size_t)c * SH_SQN_NE + r] = em->v[(size_t)c * SH_SQN_NE + r];
    for (int l = 0; l < 6; l++) {
        const int cin = l == 0 ? SH_SQN_NE : SH_SQN_NF, cout = l == 5 ? SH_SQN_NO : SH_SQN_NF, ld = l == 5 ? 4 : SH_SQN_NF;
        float *W = t.data() + (l == 0 ? sqn_off_c1(WL) : sqn_off_res(WL, l - 1)), *b = W + (size_t)WL * cin * ld;
        for (int f = 0; f < cout; f++) {
            for (int k = 0; k < WL * cin; k++) W[(size_t)k * ld + f] = cw[l]->v[(size_t)f * WL * cin + k];      /* k = tap * cin + feature */
            b[f] = cb[l]->v[(size_t)f];
        }
    }
    m->WL = WL; m->F = SH_SQN_NF; m->S = 0; m->NS = SH_SQN_NO; m->min_samples = (size_t)(WL - 1);
    return upload(m->sqw, t);
}

extern "C" size_t scrappie_hip_sqnet_tile(void) { return SH_SQN_TP; }

static std::atomic<uint64_t> g_sqnet_launches;
extern "C" uint64_t scrappie_hip_sqnet_launch_count(void) { return g_sqnet_launches.load(std::memory_order_relaxed); }

extern "C" void scrappie_hip_sqnet_timing(scrappie_hip_engine *e, double out[3]) { timing3(e ? e->sqnet_ms : nullptr, out); }

/* the reference's undefined calls (layers.c:190-241: below WL - 1 columns the edge products of `convolution` read outside X; embedding asserts
 * its codes): 0, or -1 with the reason */
static int sqnet_seq_ok(const char *fn, const int *seq, size_t n, int WL) {
    if (!seq) return set_err("%s: no sequence", fn);
    if (n + 1 < (size_t)WL) return set_err("%s: a sequence of %zu bases is shorter than the %d a window of %d needs", fn, n, WL - 1, WL);
    if (n > (size_t)INT32_MAX / 2) return set_err("%s: %zu bases is too many", fn, n);
    for (size_t i = 0; i < n; i++)
        if (seq[i] < 0 || seq[i] > 3) return set_err("%s: code %d at base %zu is outside 0..3", fn, seq[i], i);
    return 0;
}

static void sqnet_transform(float *col) {      /* networks.c:440-448 */
    col[1] = expf(col[1]);
    col[2] = expf(-col[2]);
}

/* device bytes a sequence of n bases adds to a launch: codes, outputs, tiles */
static size_t sqnet_seq_bytes(size_t n) { return n + n * SH_SQN_NO * 4 + ((n + SH_SQN_TP - 1) / SH_SQN_TP) * sizeof(ShSqnetTile) + 64; }

/* one launch over the sequences who[0 .. nw) of the call */
static int sqnet_run(scrappie_hip_engine *e, const Model *m, const std::vector<size_t> &who, const int *const *seqs, const size_t *n, int transform_units,
                     scrappie_matrix *out) {
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    DBuf *d = e->d_sqn;           /* 0 tiles | codes, 1 outputs */
    const auto t0 = std::chrono::steady_clock::now();
    size_t nbase = 0, ntile = 0;
    for (size_t i : who) { nbase += n[i]; ntile += (n[i] + SH_SQN_TP - 1) / SH_SQN_TP; }
    const size_t tile_bytes = ntile * sizeof(ShSqnetTile);
    if (d[0].ensure(tile_bytes + nbase + 16) || d[1].ensure(nbase * SH_SQN_NO * 4 + 16) ||
        e->h_sqn.ensure(std::max(tile_bytes + nbase, nbase * SH_SQN_NO * 4) + 16)) return -1;
    /* staging (pinned): tiles | codes, one upload */
    ShSqnetTile *ht = e->h_sqn.as<ShSqnetTile>();
    unsigned char *hc = (unsigned char *)(ht + ntile);
    size_t off = 0, kt = 0;
    for (size_t i : who) {
        for (size_t t = 0; t < n[i]; t += SH_SQN_TP) ht[kt++] = ShSqnetTile{(long long)off, (int)n[i], (int)t};
        for (size_t k = 0; k < n[i]; k++) hc[off + k] = (unsigned char)seqs[i][k];
        off += n[i];
    }
    HIPCHK(hipMemcpyAsync(d[0].p, ht, tile_bytes + nbase, hipMemcpyHostToDevice, s));
    HIPCHK(sh_stream_wait(s));
    ShSqnetArgs a{};
    a.tile = d[0].as<ShSqnetTile>(); a.code = d[0].as<unsigned char>() + tile_bytes; a.w = m->sqw.as<float>(); a.out = d[1].as<float>();
    const auto t1 = std::chrono::steady_clock::now();
    g_sqnet_launches.fetch_add(1, std::memory_order_relaxed);
    if (pick_bool([&](auto w9) { return launch_k<k_sqnet<w9() ? 9 : 7>>(dim3((unsigned)ntile), dim3(SH_SQN_NTH), 0, s, a); }, m->WL == 9)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    const auto t2 = std::chrono::steady_clock::now();
    float *ho = e->h_sqn.as<float>();
    HIPCHK(hipMemcpyAsync(ho, d[1].p, nbase * SH_SQN_NO * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    off = 0;
    for (size_t i : who) {
        scrappie_matrix mat = make_scrappie_matrix(SH_SQN_NO, n[i]);        /* zeroed: the pad lane stays 0 */
        if (!mat) return set_err("out of host memory");
        out[i] = mat;
        for (size_t c = 0; c < n[i]; c++) {
            float *col = mat->data.f + c * mat->stride;
            memcpy(col, ho + (off + c) * SH_SQN_NO, SH_SQN_NO * 4);
            if (transform_units) sqnet_transform(col);
        }
        off += n[i];
    }
    const auto t3 = std::chrono::steady_clock::now();
    e->sqnet_ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    e->sqnet_ms[1] += std::chrono::duration<double, std::milli>(t2 - t1).count();
    e->sqnet_ms[2] += std::chrono::duration<double, std::milli>(t3 - t2).count();
    return 0;
}

extern "C" int scrappie_hip_squiggle_predict_batch(scrappie_hip_engine *e, const char *model, const int *const *seqs, const size_t *n, size_t count,
                                                   int transform_units, scrappie_matrix *out) {
    if (!e || !model || (count && (!seqs || !n || !out))) return set_err("squiggle_predict_batch: null argument");
    for (size_t i = 0; i < count; i++) out[i] = nullptr;
    const int h = scrappie_hip_find_model(e, model);
    if (h < 0) return set_err("squiggle_predict_batch: model '%s' is not loaded on this engine", model);
    const Model *m = e->models[(size_t)h];
    if (m->arch != 4) return set_err("squiggle_predict_batch: model '%s' is not a squiggle model", model);
    (void)hipSetDevice(e->device);
    { std::lock_guard<std::mutex> lk(e->mu); for (double &x : e->sqnet_ms) x = 0.0; }
    const size_t budget = launch_budget(e, e->dbg_sqnet_budget);
    struct Load { size_t bytes = 0, tiles = 0; };
    LaunchCut<Load> cut{e, "squiggle_predict_batch"};
    cut.run = [&](const std::vector<size_t> &who, Load &) { return sqnet_run(e, m, who, seqs, n, transform_units, out); };
    for (size_t i = 0; i < count && !cut.failed; i++) {
        if (sqnet_seq_ok("squiggle_predict_batch", seqs[i], n[i], m->WL)) { cut.refuse(i, g_err); continue; }
        const size_t sb = sqnet_seq_bytes(n[i]), st = (n[i] + SH_SQN_TP - 1) / SH_SQN_TP;
        if (sb > budget) {
            char msg[200];
            snprintf(msg, sizeof msg, "squiggle_predict_batch: %zu bases need %zu bytes on the device, more than one launch may take (%zu)", n[i], sb, budget);
            cut.refuse(i, msg);
            continue;
        }
        cut.add(i, cut.load.bytes + sb <= budget && cut.load.tiles + st <= (size_t)INT32_MAX / 2);
        cut.load.bytes += sb; cut.load.tiles += st;
    }
    return cut.finish([&] { for (size_t i = 0; i < count; i++) out[i] = free_scrappie_matrix(out[i]); },
                      [](size_t i, const char *why) { set_err("%s (sequence %zu of the call)", why, i); });
}

/* ------------------------------------------------------------------ */
/* per-read reference surface (networks.c:397, :454, :511)              */
/* ------------------------------------------------------------------ */
static scrappie_matrix sqnet_one(const char *name, int WL, const int *sequence, size_t n, bool transform_units) {
    if (sqnet_seq_ok(name, sequence, n, WL)) return nullptr;
    {   /* a model nobody has registered: said before an engine is asked for */
        std::lock_guard<std::mutex> lk(g_models_mu);
        if (g_models.find(name) == g_models.end() && !getenv("SCRAPPIE_MODEL_DIR")) {
            set_err("model '%s' is not registered and SCRAPPIE_MODEL_DIR is unset (weights are not compiled in)", name);
            return nullptr;
        }
    }
    scrappie_hip_engine *e = default_engine();
    if (!e) return nullptr;
    const int h = default_model(e, name);
    if (h < 0) return nullptr;
    const Model *m = e->models[(size_t)h];
    if (m->arch != 4 || m->WL != WL) {
        set_err("%s: the model registered under this name is not a squiggle model with a window of %d", name, WL);
        return nullptr;
    }
    scrappie_matrix out = nullptr;
    if (scrappie_hip_squiggle_predict_batch(e, name, &sequence, &n, 1, transform_units ? 1 : 0, &out)) return nullptr;
    return out;
}

extern "C" scrappie_matrix squiggle_r94(int const *sequence, size_t n, bool transform_units) { return sqnet_one("squiggle_r94", 9, sequence, n, transform_units); }
extern "C" scrappie_matrix squiggle_r94_rna(int const *sequence, size_t n, bool transform_units) { return sqnet_one("squiggle_r94_rna", 7, sequence, n, transform_units); }
extern "C" scrappie_matrix squiggle_r10(int const *sequence, size_t n, bool transform_units) { return sqnet_one("squiggle_r10", 9, sequence, n, transform_units); }
