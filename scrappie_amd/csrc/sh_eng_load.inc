/* sh_eng_load.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * the .scrm container -> Model, engine settings, the planning functions of the ABI. */

/* -------------------- .scrm container (scrappie_amd/model.py) -------- */
static const HostMat *find_mat(const std::vector<std::pair<std::string, HostMat>> &ms, const char *nm) {
    for (auto &kv : ms) if (kv.first == nm) return &kv.second;
    return nullptr;
}

static int load_model_mem_one(scrappie_hip_engine *e, const char *name, const void *blob, size_t nbytes);
static int sqnet_load(Model *m, const std::vector<std::pair<std::string, HostMat>> &mats);      /* sh_eng_sqnet.inc */
extern "C" int scrappie_hip_load_model_mem(scrappie_hip_engine *e, const char *name, const void *blob, size_t nbytes) {
    const int idx = load_model_mem_one(e, name, blob, nbytes);
    if (idx < 0 || e->is_tail) return idx;
    /* kept, so that the helper engine for chain-bound reads (scrappie_hip_basecall_batch) can be given the same models at the same indices */
    scrappie_hip_engine::Blob b{name, std::vector<unsigned char>((const unsigned char *)blob, (const unsigned char *)blob + nbytes), e->dbg_force_f32};
    bool found = false;
    for (auto &x : e->blobs) if (x.name == b.name) { x = b; found = true; }
    if (!found) e->blobs.push_back(b);
    if (e->tail || e->tail2) {      /* a helper may still be running a deferred ticket (its worker reads helper->models): wait until both are idle */
        std::unique_lock<std::mutex> lk(e->tail_mu);
        e->tail_cv.wait(lk, [&] { return e->tail_busy == 0 && e->tail_q.empty(); });
    }
    for (scrappie_hip_engine **tp : {&e->tail, &e->tail2}) if (*tp) {
        (*tp)->dbg_force_f32 = e->dbg_force_f32;
        if (load_model_mem_one(*tp, name, blob, nbytes) != idx) return set_err("model '%s' did not load at the same index on the helper engine", name);
    }
    return idx;
}
static int load_model_mem_one(scrappie_hip_engine *e, const char *name, const void *blob, size_t nbytes) {
    if (!e || !name || !blob) return set_err("load_model: null argument");
    const unsigned char *p = (const unsigned char *)blob, *end = p + nbytes;
    if (nbytes < 24 || memcmp(p, "SCRMDL01", 8) != 0) return set_err("model '%s': not a .scrm container", name);
    uint32_t hdr[4];
    memcpy(hdr, p + 8, 16);
    p += 24;
    std::vector<std::pair<std::string, HostMat>> mats;
    for (uint32_t i = 0; i < hdr[3]; i++) {
        if (p + 40 > end) return set_err("model '%s': truncated", name);
        char nm[33]; memcpy(nm, p, 32); nm[32] = 0;
        uint32_t nr, nc; memcpy(&nr, p + 32, 4); memcpy(&nc, p + 36, 4);
        p += 40;
        const size_t cnt = (size_t)nr * nc;
        if (p + cnt * 4 > end) return set_err("model '%s': truncated matrix %s", name, nm);
        HostMat hm; hm.nr = (int)nr; hm.nc = (int)nc; hm.v.resize(cnt);
        memcpy(hm.v.data(), p, cnt * 4);
        p += cnt * 4;
        mats.emplace_back(nm, std::move(hm));
    }
    (void)hipSetDevice(e->device);
    Model *m = new Model();
    m->name = name;
    m->arch = (int)hdr[0]; m->conv_act = (int)hdr[1]; m->stride = (int)hdr[2];
    const HostMat *cw = find_mat(mats, "conv_W"), *cb = find_mat(mats, "conv_b");
    const HostMat *fw = find_mat(mats, "ff_W"), *fb = find_mat(mats, "ff_b");
    if (m->arch == 3) {
        /* events bi-LSTM (networks.c:146-193): no convolution; lstm0..3 = F1, B1, F2, B2 */
        if (!fw || !fb) { delete m; return set_err("model '%s': missing ff matrices", name); }
        m->NS = fw->nc; m->S = fw->nr; m->stride = 1; m->WL = 0;
        const HostMat *i0 = find_mat(mats, "lstm0_iW");
        m->nfeat = i0 ? i0->nr : 0;
        m->F = 16;
        if (!i0 || m->nfeat < 1 || m->nfeat > 16 || m->S % 32 != 0 || m->S > 96 || (m->NS - 1) % 64 != 0) {
            delete m; return set_err("model '%s': unsupported events dims features=%d S=%d NS=%d", name, m->nfeat, m->S, m->NS);
        }
        for (int l = 0; l < 4; l++) {
            char nm[32];
            const HostMat *mi, *ms, *mb, *mpp;
            snprintf(nm, sizeof nm, "lstm%d_iW", l); mi = find_mat(mats, nm);
            snprintf(nm, sizeof nm, "lstm%d_sW", l); ms = find_mat(mats, nm);
            snprintf(nm, sizeof nm, "lstm%d_b", l); mb = find_mat(mats, nm);
            snprintf(nm, sizeof nm, "lstm%d_p", l); mpp = find_mat(mats, nm);
            const int I = (l < 2) ? m->nfeat : m->S;
            if (!mi || !ms || !mb || !mpp || mi->nr != I || mi->nc != 4 * m->S || ms->nr != m->S || ms->nc != 4 * m->S ||
                mb->nr * mb->nc != 4 * m->S || mpp->nr * mpp->nc != 3 * m->S) {
                delete m;
                return set_err("model '%s': LSTM layer %d has wrong shapes", name, l);
            }
            for (const HostMat *x : {mi, ms}) if (!in_split_range(*x)) {
                const float mx = max_abs(*x);
                delete m;
                return set_err("model '%s': LSTM layer %d has a weight of magnitude %g, outside the split products' range (< %g); "
                               "there is no exact-fp32 LSTM kernel", name, l, mx, (double)SH_W_LIMIT);
            }
            HostMat padded;                                  /* first level: K padded from 12 to 16 with zeros */
            const HostMat *src = mi;
            if (I % 16 != 0) {
                padded.nr = 16; padded.nc = mi->nc; padded.v.assign((size_t)16 * mi->nc, 0.0f);
                for (int c = 0; c < mi->nc; c++) for (int r = 0; r < I; r++) padded.v[(size_t)c * 16 + r] = mi->v[(size_t)c * I + r];
                src = &padded;
            }
            int mt, mtp;
            int mt_s;
            if (upload(m->iW[l], make_frags(*src, mt)) || upload(m->ib[l], make_bias_frags(*mb, mt)) ||
                upload(m->sW[l], make_frags(*ms, mt_s))) { delete m; return -1; }
            HostMat padded32;                                /* ... and to one 32-wide k step for the split products of k_lstm_proj */
            const HostMat *psrc = src;
            if (src->nr % 32 != 0) {
                padded32.nr = 32; padded32.nc = mi->nc; padded32.v.assign((size_t)32 * mi->nc, 0.0f);
                for (int c = 0; c < mi->nc; c++) for (int r = 0; r < I; r++) padded32.v[(size_t)c * 32 + r] = mi->v[(size_t)c * I + r];
                psrc = &padded32;
            }
            if (upload_u32(m->iWp[l], make_piece_frags(*psrc)) || upload(m->ibs[l], scaled(make_bias_frags(*mb, mt), SH_OSCALE))) { delete m; return -1; }
            if (upload_u32(m->sWp[l], make_piece_frags(*ms))) { delete m; return -1; }
            mtp = 3 * m->S / 16;
            if (upload(m->lp[l], make_bias_frags(*mpp, mtp))) { delete m; return -1; }
        }
    } else if (m->arch == 4) {
        /* the squiggle predictor (networks.c:397-565): no recurrent layers, no output layer; WL from the shapes */
        if (sqnet_load(m, mats)) { delete m; return -1; }
        std::lock_guard<std::mutex> lk(e->mu);
        for (size_t i = 0; i < e->models.size(); i++)
            if (e->models[i]->name == name) { delete e->models[i]; e->models[i] = m; return (int)i; }
        e->models.push_back(m);
        return (int)e->models.size() - 1;
    } else {
    if (!cw || !cb || !fw || !fb) { delete m; return set_err("model '%s': missing conv/ff matrices", name); }
    m->WL = cw->nr; m->F = cw->nc; m->NS = fw->nc; m->S = fw->nr;
    bool ok = (m->F % 16 == 0) && (m->S % 16 == 0) && m->stride > 0 && m->WL > 0;
    if (m->arch == 1) ok = ok && (m->F == m->S) && m->NS == 25;          /* residuals: layers.c:286-288 */
    /* the NETWORK runs for any number of states (softmax_with_temperature, layers.c:340-357: row_normalise_inplace masks the padding of the last
     * vector whatever nr is -- src/test/test_scrappie_matrix.c:24-51 pins nr = 8 ... 11); it is decode_transducer that needs 4^k k-mers + stay
     * (decode.c:132-138), and that is refused where it is asked for (launch_viterbi) */
    if (m->arch == 0 || m->arch == 2) ok = ok && m->NS >= 2;
    if (m->arch > 3) ok = false;
    if (!ok) { delete m; return set_err("model '%s': unsupported dims F=%d S=%d NS=%d WL=%d", name, m->F, m->S, m->NS, m->WL); }
    {   /* conv taps as [WL][F] so 4 consecutive filters load as one vector */
        std::vector<float> w((size_t)m->WL * m->F);
        for (int f = 0; f < m->F; f++) for (int t = 0; t < m->WL; t++) w[(size_t)t * m->F + f] = cw->v[(size_t)f * m->WL + t];
        if (upload(m->conv_W, w) || upload(m->conv_b, cb->v)) { delete m; return -1; }
    }
    const int ngru = (m->arch == 2) ? 4 : 5;
    for (int l = 0; l < ngru; l++) {
        char nm[32];
        const HostMat *mi, *ms, *ms2, *mb;
        snprintf(nm, sizeof nm, "gru%d_iW", l); mi = find_mat(mats, nm);
        snprintf(nm, sizeof nm, "gru%d_sW", l); ms = find_mat(mats, nm);
        snprintf(nm, sizeof nm, "gru%d_sW2", l); ms2 = find_mat(mats, nm);
        snprintf(nm, sizeof nm, "gru%d_b", l); mb = find_mat(mats, nm);
        const int I = (m->arch == 2) ? (l < 2 ? m->F : m->S) : ((l == 0) ? m->F : m->S);
        if (!mi || !ms || !ms2 || !mb || mi->nr != I || mi->nc != 3 * m->S || ms->nr != m->S || ms->nc != 2 * m->S ||
            ms2->nr != m->S || ms2->nc != m->S || mb->nr * mb->nc != 3 * m->S) {
            delete m;
            return set_err("model '%s': GRU layer %d has wrong shapes", name, l);
        }
        /* a weight the fp16 pieces cannot hold (|w| >= 255): this layer runs on the exact-fp32 kernels
         * (k_affine<.., F32> + k_gru_lanes / k_gru) instead -- slower, same results as the reference's fp32 */
        m->layer_f32[l] = !(in_split_range(*mi) && in_split_range(*ms) && in_split_range(*ms2)) || e->dbg_force_f32;
        if (m->layer_f32[l] && !(std::isfinite(max_abs(*mi)) && std::isfinite(max_abs(*ms)) && std::isfinite(max_abs(*ms2)))) {
            delete m;
            return set_err("model '%s': GRU layer %d holds a non-finite weight", name, l);
        }
        if (m->layer_f32[l] && !e->dbg_force_f32)
            fprintf(stderr, "scrappie_hip: model '%s' GRU layer %d has |w| >= %g: outside the split products' operand range, using the exact-fp32 kernels for it\n",
                    name, l, (double)SH_W_LIMIT);
        int mt, mt_s;
        std::vector<float> ifr = make_frags(*mi, mt);
        if (upload(m->iW[l], ifr) || upload(m->ib[l], make_bias_frags(*mb, mt)) ||
            upload(m->sW[l], make_frags(*ms, mt_s)) || upload(m->sW2[l], make_frags(*ms2, mt_s))) { delete m; return -1; }
        if ((mi->nr % 32 == 0 && (upload_u32(m->iWp[l], make_piece_frags(*mi)) || upload(m->ibs[l], scaled(make_bias_frags(*mb, mt), SH_OSCALE)))) ||
            (m->S % 32 == 0 && (upload_u32(m->sWp[l], make_piece_frags(*ms)) || upload_u32(m->sW2p[l], make_piece_frags(*ms2))))) { delete m; return -1; }
#ifdef SH_EXPERIMENTS
        if (m->S == 96 && I == 96 && !m->layer_f32[l]) {      /* k_gru_proj32 */
            if (upload_u32(m->iWp32[l], make_piece_frags32(*mi)) || upload_u32(m->sWp32[l], make_piece_frags32(*ms)) ||
                upload_u32(m->sW2p32[l], make_piece_frags32(*ms2)) || upload(m->ib32[l], make_bias32(*mb))) { delete m; return -1; }
            m->has32 = true;
        }
#endif
    }
    }
    if (m->arch == 2 || m->arch == 3) {   /* the two joining layers: misc/parse_raw.py:93-99,121-126; networks.c:167,180 */
        for (int k = 0; k < 2; k++) {
            char nm[32];
            const HostMat *wf, *wb, *bb;
            snprintf(nm, sizeof nm, "ff%d_Wf", k + 1); wf = find_mat(mats, nm);
            snprintf(nm, sizeof nm, "ff%d_Wb", k + 1); wb = find_mat(mats, nm);
            snprintf(nm, sizeof nm, "ff%d_b", k + 1); bb = find_mat(mats, nm);
            if (!wf || !wb || !bb || wf->nr != m->S || wb->nr != m->S || wf->nc != m->S || wb->nc != m->S || bb->nr * bb->nc != m->S) {
                delete m;
                return set_err("model '%s': FF%d has wrong shapes (need S x S)", name, k + 1);
            }
            for (const HostMat *x : {wf, wb}) if (!in_split_range(*x)) {
                const float mx = max_abs(*x);
                delete m;
                return set_err("model '%s': FF%d has a weight of magnitude %g, outside the split products' range (< %g); "
                               "there is no exact-fp32 kernel for this layer", name, k + 1, mx, (double)SH_W_LIMIT);
            }
            const int mt = (m->S + 15) / 16;
            /* as fp16 pieces (split products), the bias in accumulator units */
            if (upload_u32(m->ff2W[k][0], make_piece_frags(*wf)) || upload_u32(m->ff2W[k][1], make_piece_frags(*wb)) ||
                upload(m->ff2b[k], scaled(make_bias_frags(*bb, mt), SH_OSCALE))) { delete m; return -1; }
        }
    }
    if (m->S % 32 == 0 && !in_split_range(*fw)) {
        const float mx = max_abs(*fw);
        delete m;
        return set_err("model '%s': the output layer has a weight of magnitude %g, outside the split products' range (< %g); "
                       "there is no exact-fp32 kernel for this layer", name, mx, (double)SH_W_LIMIT);
    }
    {   /* exp_ps clamps its argument to +-88.3762626647949 (sse_mathfun.h:233-234).  The output layer reads the trunk's last layer -- a GRU state, a tanh or
         * o * tanh(c): |x| <= 1 -- so |logit of state s| <= sum_k |W[k][s]| + |b[s]|; where that stays below 88 for every state the clamp can never act and
         * the fused S1 (k_ff_viterbi_teams) leaves the v_med3_f32 out: one of its four VALU instructions per value, same bits (the kernel is bound by
         * the instructions its SIMDs issue: profiles/r6_dual_issue.txt).  Temperatures other than 1 and the trunk-input hook keep the clamp. */
        double worst = 0.0;
        for (int c = 0; c < fw->nc; c++) {
            double acc = c < (int)fb->v.size() ? fabs((double)fb->v[(size_t)c]) : 0.0;
            for (int r = 0; r < fw->nr; r++) acc += fabs((double)fw->v[(size_t)c * fw->nr + r]);
            worst = std::max(worst, acc);
        }
        m->ff_no_clamp = worst < 88.0;
    }
    if (upload(m->ffW, make_frags(*fw, m->ff_mtiles)) || upload(m->ffb, make_bias_frags(*fb, m->ff_mtiles))) { delete m; return -1; }
    if (m->S % 32 == 0 && (upload_u32(m->ffWp, make_piece_frags(*fw)) || upload(m->ffbs, scaled(make_bias_frags(*fb, m->ff_mtiles), SH_OSCALE)))) { delete m; return -1; }
    if (m->arch == 3) {
        m->min_samples = 2;                       /* lstm_forward needs two columns (layers.c:697) */
    } else {
    /* conv geometry: layers.c:169-207 */
    ShConvGeom &g = m->geom;
    g = conv_geom(m->WL, m->stride, m->F);
    /* below this the reference's edge arithmetic under/overflows (layers.c:227-231)
     * and gru_forward needs two columns (layers.c:400) */
    m->min_samples = (size_t)(g.shiftX + 2 * g.nstepX + g.WL);
    if (m->min_samples < (size_t)(g.st + 1)) m->min_samples = (size_t)(g.st + 1);
    }
    std::lock_guard<std::mutex> lk(e->mu);
    for (size_t i = 0; i < e->models.size(); i++)
        if (e->models[i]->name == name) { delete e->models[i]; e->models[i] = m; return (int)i; }
    e->models.push_back(m);
    return (int)e->models.size() - 1;
}

extern "C" int scrappie_hip_load_model(scrappie_hip_engine *e, const char *name, const char *path) {
    if (!path) return set_err("load_model: null path");
    FILE *fh = fopen(path, "rb");
    if (!fh) return set_err("cannot open model file %s", path);
    fseek(fh, 0, SEEK_END);
    long sz = ftell(fh);
    fseek(fh, 0, SEEK_SET);
    std::vector<unsigned char> buf((size_t)std::max(0L, sz));
    const size_t got = fread(buf.data(), 1, buf.size(), fh);
    fclose(fh);
    if (got != buf.size()) return set_err("short read on %s", path);
    return scrappie_hip_load_model_mem(e, name, buf.data(), buf.size());
}

extern "C" int scrappie_hip_find_model(scrappie_hip_engine *e, const char *name) {
    if (!e || !name) return -1;
    std::lock_guard<std::mutex> lk(e->mu);
    for (size_t i = 0; i < e->models.size(); i++) if (e->models[i]->name == name) return (int)i;
    return -1;
}

static Model *get_model(scrappie_hip_engine *e, int model) {
    if (!e || model < 0 || (size_t)model >= e->models.size()) { set_err("invalid model handle %d", model); return nullptr; }
    if (e->models[model]->arch == 4) { set_err("model '%s' predicts squiggles from sequences; it takes no signal", e->models[model]->name.c_str()); return nullptr; }
    return e->models[model];
}

extern "C" size_t scrappie_hip_min_samples(scrappie_hip_engine *e, int model) {
    Model *m = get_model(e, model);
    return m ? m->min_samples : 0;
}
extern "C" int scrappie_hip_model_stride(scrappie_hip_engine *e, int model) {
    Model *m = get_model(e, model);
    return m ? m->stride : -1;
}
extern "C" void scrappie_hip_set_profiling(scrappie_hip_engine *e, int on) { if (e) e->profiling = on != 0; }
static int resolve_spans(scrappie_hip_engine *e, Slot &sl) {
    /* all events of the slot have completed (caller waited on its done event or drained the stream) */
    scrappie_hip_timing &tm = sl.timing;
    float dbg_wait = 0.f, dbg_lead = 0.f;
    float *fields[F_COUNT] = {&tm.conv_ms, &tm.affine_ms, &tm.gru_ms, &tm.ff_ms, &tm.decode_ms, &tm.backtrace_ms, &tm.total_ms, &tm.fused_ms, &tm.stitch_ms,
                              &dbg_wait, &dbg_lead};      /* in the order of SpanField */
    for (auto &sp : sl.spans) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, sl.ev[sp.i], sl.ev[sp.j]));
        *fields[sp.field] += ms;
    }
    sl.spans.clear();
    if (tun().host_stamp) fprintf(stderr, "host stamp: main stream waited %.2f ms for the prologue; the convolution had ended %.2f ms before the main stream got there (negative: after)\n", dbg_wait, dbg_lead);
    e->timing = tm;
    return 0;
}

/* timing of the launch group most recently collected (or, if none was collected
 * since, of the most recent run once the stream has drained) */
extern "C" int scrappie_hip_get_timing(scrappie_hip_engine *e, scrappie_hip_timing *t) {
    if (!e || !t) return -1;
    (void)hipSetDevice(e->device);
    Slot &sl = e->current();
    if (!sl.spans.empty() && !sl.pending) {
        HIPCHK(sh_stream_wait(e->stream));
        if (resolve_spans(e, sl)) return -1;
    }
    *t = e->timing;
    return 0;
}
extern "C" void scrappie_hip_set_max_launch_reads(scrappie_hip_engine *e, size_t n) { if (e && n >= 16) e->max_launch_reads = n; }      /* (the helpers take the engine's settings with every call) */
extern "C" void scrappie_hip_set_max_launch_blocks(scrappie_hip_engine *e, size_t n) { if (e) e->max_launch_blocks = n; }
extern "C" void *scrappie_hip_device_alloc(scrappie_hip_engine *e, size_t nbytes) {
    if (!e) return nullptr;
    (void)hipSetDevice(e->device);
    void *p = nullptr;
    if (hipMalloc(&p, nbytes) != hipSuccess) { set_err("hipMalloc(%zu) failed", nbytes); return nullptr; }
    return p;
}
extern "C" void scrappie_hip_device_free(scrappie_hip_engine *e, void *dptr) {
    if (e && dptr) { (void)hipSetDevice(e->device); (void)hipFree(dptr); }
}
extern "C" int scrappie_hip_memcpy_h2d(scrappie_hip_engine *e, void *dst, const void *src, size_t nbytes) {
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    HIPCHK(hipMemcpy(dst, src, nbytes, hipMemcpyHostToDevice));
    return 0;
}
extern "C" int scrappie_hip_synchronize(scrappie_hip_engine *e) {
    if (!e) return -1;
    (void)hipSetDevice(e->device);
    HIPCHK(sh_stream_wait(e->stream));
    return 0;
}

/* The recurrent kernels' lane schedule, exposed for tests and introspection (host only, no device
 * needed): lanes_per_wg = 1 (k_gru_proj) or 2 (k_gru_split, k_lstm_lanes; = scrappie_hip_gru_schedule).
 * lane_off needs lanes_per_wg * ncu + 1 ints, seg takes cap rows of
 * {tile, first step, end step, 0}.  Returns the number of segments (even if > cap). */
extern "C" long scrappie_hip_lane_schedule(const int *tile_T, size_t ntile, int ncu, int lanes_per_wg, int *nwg, int *capacity,
                                           int *lane_off, int *seg, size_t cap) {
    if (!tile_T || ncu < 1 || lanes_per_wg < 1 || lanes_per_wg > 2) return -1;
    ShGruSchedule sc;
    sh_lane_schedule(tile_T, ntile, ncu, lanes_per_wg, sc);
    if (nwg) *nwg = sc.nwg;
    if (capacity) *capacity = sc.capacity;
    if (lane_off) memcpy(lane_off, sc.lane_off.data(), sc.lane_off.size() * sizeof(int));
    if (seg) for (size_t i = 0; i < sc.seg.size() && i < cap; i++) memcpy(seg + 4 * i, &sc.seg[i], 16);
    return (long)sc.seg.size();
}

extern "C" long scrappie_hip_gru_schedule(const int *tile_T, size_t ntile, int ncu, int *nwg, int *capacity,
                                          int *lane_off, int *seg, size_t cap) {
    return scrappie_hip_lane_schedule(tile_T, ntile, ncu, 2, nwg, capacity, lane_off, seg, cap);
}

/* The decoder's pieces (sh_sched.h), host only: seg takes cap rows of {tile, first block,
 * end block, 0}, in workgroup order.  Returns the number of pieces (even if > cap). */
extern "C" long scrappie_hip_decoder_pieces(const int *tile_T, size_t ntile, int ncu, int *seg, size_t cap) {
    if (!tile_T || ncu < 1) return -1;
    std::vector<ShGruSeg> v;
    sh_piece_schedule(tile_T, ntile, ncu, v);
    if (seg) for (size_t i = 0; i < v.size() && i < cap; i++) memcpy(seg + 4 * i, &v[i], 16);
    return (long)v.size();
}

/* The lane layout of the two-team decoder (sh_decoder_lanes, sh_sched.h), host only: one lane per workgroup; lane_off needs ncu + 1
 * ints, seg takes cap rows of {tile, first block, end block, ordinal of the segment within its tile}, each lane's segments in the order
 * they run.  capacity: M in blocks.  Returns the number of segments (even if > cap). */
extern "C" long scrappie_hip_decoder_lanes(const int *tile_T, size_t ntile, int ncu, int *nwg, int *capacity, int *lane_off, int *seg, size_t cap) {
    if (!tile_T || ncu < 1) return -1;
    ShGruSchedule sc;
    sh_decoder_lanes(tile_T, ntile, ncu, sc);
    if (nwg) *nwg = sc.nwg;
    if (capacity) *capacity = sc.capacity;
    if (lane_off) memcpy(lane_off, sc.lane_off.data(), sc.lane_off.size() * sizeof(int));
    if (seg) for (size_t i = 0; i < sc.seg.size() && i < cap; i++) memcpy(seg + 4 * i, &sc.seg[i], 16);
    return (long)sc.seg.size();
}

/* Cut a list of reads (input order kept) into launch groups of at most max_reads reads and at most
 * max_blocks column blocks (16 reads x 1 block; what the device arena is proportional to).  Tiles are
 * formed from reads sorted by length inside a group, so a group's column blocks are bounded by
 * sum(T)/16 + max(T).  Host only.  starts takes cap group start indices; returns the number of groups
 * (even if > cap), or -1 when a single read alone exceeds max_blocks. */
extern "C" long scrappie_hip_plan_groups(const uint32_t *lengths, size_t n, int stride, size_t max_reads, size_t max_blocks,
                                         size_t *starts, size_t cap) {
    if ((!lengths && n) || stride < 1 || max_reads < 1) return -1;
    long ng = 0;
    size_t cnt = 0;
    unsigned long long sumT = 0, maxT = 0;
    for (size_t i = 0; i < n; i++) {
        const unsigned long long T = ((unsigned long long)lengths[i] + stride - 1) / stride;
        if (max_blocks && T / 16 + T + 1 > max_blocks) return -1;
        const unsigned long long ns = sumT + T, nm = std::max(maxT, T);
        if (cnt == 0 || cnt >= max_reads || (max_blocks && ns / 16 + nm + 1 > max_blocks)) {
            if (starts && (size_t)ng < cap) starts[ng] = i;
            ng++;
            cnt = 0; sumT = 0; maxT = 0;
        }
        cnt++; sumT += T; maxT = std::max(maxT, T);
    }
    return ng;
}

/* S1 inside the decoder (k_ff_viterbi): the posterior of a basecall is never written.  Whenever somebody wants to see
 * it (scrappie_hip_posterior, the decoder-input hook) or the shape is not the 4^5 + 1 states over 96 units the kernel
 * is built for, the two-kernel form runs instead -- with identical bits. */
static bool decoder_fused(const scrappie_hip_engine *e, const Model *m) {
    return m->NS > 25 && !e->alt_prob && m->NS == 1025 && m->S == 96 && !tun().ff_separate && !e->dbg_ff_separate;
}

/* device bytes one column block costs across the arena (activations x3, gate inputs where they exist, the posterior
 * where it is written, traceback, per-slot result buffers x2, signals x2): what bounds a launch group on a 288 GB part */
static size_t bytes_per_block(const Model *m, bool posterior) {
    const size_t S = (size_t)m->S, F = (size_t)m->F, w = std::max(S, F);
    /* activation buffers: the convolution's output per slot (2) + the layers' ping-pong partner; the bi-directional stacks
     * (raw_r94, events) keep a third layer buffer */
    size_t b = ((m->arch == 2 || m->arch == 3) ? 4 : 3) * w * 64 + 128;
    if (posterior) b += (size_t)m->ff_mtiles * 1024;
    if (m->arch == 3 || F != S || S % 32 || S / 16 > 6) b += (size_t)(m->arch == 3 ? 4 : 3) * S * 64;   /* gate inputs in HBM */
    if (m->NS > 25) b += (size_t)((m->NS - 1) / 4) * 64;     /* transducer traceback: one byte per state */
    else b += 16 * 4 * 4;
    /* per slot: path + position (4 + 4 bytes per read and block), side rows of the homopolymer correction (20), bases (5) */
    b += 16 * 2 * (4 + 4 + 20 + 5) + 2 * 16 * 4 * (size_t)std::max(m->stride, 1) * (m->arch == 3 ? (size_t)m->nfeat : 1);
    return b;
}

/* A launch group as large as the arena allows: a group lasts at least as long as its longest tile's serial chain
 * (blocks x layers), so mixed-length reads fill the device only when the group's blocks per lane reach the longest
 * tile (profiles/r3_mixed_rate_*.txt: 3000 reads of U{1000..40000} samples 6.4e8 samples/s, 16000 reads 1.44e9). */
static size_t launch_block_cap(scrappie_hip_engine *e, const Model *m) {
    if (e->max_launch_blocks) return e->max_launch_blocks;
    return (size_t)(e->mem_frac * (double)e->total_mem) / bytes_per_block(m, !decoder_fused(e, m));
}
