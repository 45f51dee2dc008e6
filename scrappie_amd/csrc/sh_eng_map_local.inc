/* sh_eng_map_local.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * reads of a transducer model mapped INTO a longer sequence of k-mer states (k_map_local, sh_map_local.h).  Two passes, as
 * sh_eng_map_crf_local.inc: every window of every read of a launch in ONE k_map_local launch (per home), scores and end states back, the
 * host picks each read's best window (or sums them); with a path wanted a second launch runs the traceback on that window alone
 * and k_map_local_walk returns path, first and last.  map_to_reference_* on the process-default engine (the caller's host posterior
 * uploaded, the dense loader) and scrappie_hip_map_post_local_batch: the network and S1 of a launch group (run_staged to STOP_POST),
 * both passes on the posterior where S1 left it in d_E, under the engine's lock.  The cut of a sequence into windows is host
 * arithmetic in sh_host.c (scrappie_hip_map_local_plan).  The windows' buffers are a DpBufs and their device order is dp_order's
 * (sh_eng_cut.inc); the upload of a host matrix, the batch call and the launch group's stage are sh_eng_post.inc's; the windows' forward
 * sum, the load of a launch group and the results' type are sh_eng_map_crf_local.inc's. */

/* launches of each k_map_local form in this process: index (vit ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_map_local_forms[8];
extern "C" void scrappie_hip_map_local_form_counts(uint64_t forms[8]) {
    if (forms) for (int i = 0; i < 8; i++) forms[i] = g_map_local_forms[i].load(std::memory_order_relaxed);
}

static const size_t POST_LOCAL_MAX_STATES = (size_t)4 * SH_MAP_NTH * SH_MAPL_PIECES;      /* what a workgroup stages of a column */

/* one read of a launch: where its posterior is (as plan_add takes it), its sequence, and what comes back */
struct PostLocalJob {
    long long post; int lane; size_t nblock;
    const int *seq; size_t L;
    float score = NAN; size_t first = (size_t)-1, last = 0; int32_t *path = nullptr;
    int2 end = make_int2(0, 0);
};

/* the windows of a sequence for a read, as the planner cuts them */
static long long post_local_cut(size_t L, size_t nblock, size_t nr, long stride, MapLocalCut *c) {
    const long long nw = scrappie_hip_map_local_plan(L, nblock, nr, stride, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!c || nw <= 0) return nw;
    const size_t n = (size_t)nw;
    c->first.resize(n); c->ncell.resize(n); c->own.resize(n); c->home.resize(n); c->scr.resize(n);
    long long fl = 0;
    return scrappie_hip_map_local_plan(L, nblock, nr, stride, n, c->first.data(), c->ncell.data(), c->own.data(), c->home.data(), c->scr.data(), &fl);
}

/* move codes (4 ceil(ncell / 64) words per block) and the END plane (half as many) */
static long long post_local_tb_words(size_t ncell, size_t nblock) { return (long long)nblock * (long long)(6 * ((ncell + 63) / 64)); }
static long long post_local_scr_floats(size_t ncell) { return (long long)(3 * ((ncell + 3) & ~(size_t)3)); }

/* device bytes one read adds to a launch, its sequence apart: the first pass's windows, scores, end states and scratch rows; with a
 * path the second pass's traceback and rows on its largest window, and the path */
static size_t post_local_read_bytes(size_t L, size_t nblock, size_t nr, long stride, bool path) {
    long long fl = 0;
    const long long nw = scrappie_hip_map_local_plan(L, nblock, nr, stride, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &fl);
    size_t b = (size_t)nw * (sizeof(ShMapLocalWin) + 12) + (size_t)fl * 4 + 64;
    if (path) {
        const size_t s = scrappie_hip_map_local_stride(L, nblock, nr, stride);
        const size_t nc = std::min(s + 2 * (nblock - 1), L);
        b += (size_t)post_local_tb_words(nc, nblock) * 4 + nblock * 4 + (size_t)post_local_scr_floats(nc) * 4 + sizeof(ShMapLocalWin) + 64;
    }
    return b;
}

/* the record of window w of job j's cut c; seq_at: where the job's codes lie in d_ml_seq; tb: its traceback's word offset, -1: none; scr_floats
 * and lds take what it needs of its home */
static ShMapLocalWin post_local_win(const PostLocalJob &j, long long seq_at, const MapLocalCut &c, size_t w, size_t nr, long long tb, long long &scr_floats,
                                    size_t &lds) {
    ShMapLocalWin r{};
    r.post = j.post; r.lane = j.lane; r.nblock = (int)j.nblock; r.seqlen = (int)j.L; r.seq = seq_at;
    r.first = (int)c.first[w]; r.ncell = (int)c.ncell[w]; r.own = (int)c.own[w]; r.ok = 1; r.tb = tb;
    if (c.home[w]) { r.scr = scr_floats; scr_floats += post_local_scr_floats(c.ncell[w]); }
    else { r.scr = -1; lds = std::max(lds, sh_map_local_lds_bytes(c.ncell[w], nr)); }
    return r;
}

/* one launch of the windows wins[] through k_map_local, in device order (dp_order: those of the LDS home first; perm[k]: which of wins[] goes
 * k-th); scores and, Viterbi, end states into dp_ml.h ([n] float, then [n] int2), which also has room for what a walk over path_len entries returns */
static int post_local_launch(scrappie_hip_engine *e, const std::vector<ShMapLocalWin> &wins, std::vector<size_t> &perm, size_t lds, long long scr_floats,
                             long long tb_words, long long path_len, ShMapLocalArgs a, bool vit, bool tiled) {
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_ml;
    const size_t n = wins.size(), n_lds = dp_order(wins, perm);
    std::vector<ShMapLocalWin> rd;                        /* (one home only: wins[] is in device order already) */
    if (n_lds && n_lds < n) { rd.resize(n); for (size_t k = 0; k < n; k++) rd[k] = wins[perm[k]]; }
    if (d.ensure(n, sizeof(ShMapLocalWin), (tb_words + 3) & ~3LL, scr_floats, path_len, n * 24 + (size_t)path_len * 4 + 16, sizeof(int2))) return -1;
    HIPCHK(hipMemcpyAsync(d.rd.p, rd.empty() ? wins.data() : rd.data(), n * sizeof(ShMapLocalWin), hipMemcpyHostToDevice, s));
    a.rd = d.rd.as<ShMapLocalWin>(); a.seq = e->d_ml_seq.as<int>(); a.tb = d.tb.as<unsigned>();
    a.scr = d.scr.as<float>(); a.score = d.score.as<float>(); a.final_state = d.final_state.as<int2>();
    if (lds > SH_MAP_LDS) return set_err("map_local: a window of %zu bytes of LDS", lds);
    if (pick_bool([&](auto v, auto tl) {
            return dp_launch<k_map_local<v(), tl(), true>, k_map_local<v(), tl(), false>>(s, a, n_lds, n, SH_MAP_NTH, lds, sh_map_local_scr_lds_bytes((size_t)a.nr),
                                                                                         g_map_local_forms + ((v() ? 4 : 0) | (tl() ? 2 : 0)));
        }, vit, tiled)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d.h.p, d.score.p, n * 4, hipMemcpyDeviceToHost, s));
    if (vit) HIPCHK(hipMemcpyAsync((char *)d.h.p + n * 4, d.final_state.p, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    return 0;
}

/* Both passes over jobs[] (under mu).  a: where the posterior is and the penalties.  A sequence several jobs point at is uploaded
 * once.  want_path: the second pass (path, first and last) on each job's best window.  t (may be NULL): t[0] += the first pass,
 * t[1] += the second pass, the walk and the copies. */
static int post_local_run(scrappie_hip_engine *e, std::vector<PostLocalJob> &jobs, const ShMapLocalArgs &a, bool vit, bool tiled, bool want_path, double *t) {
    const size_t nj = jobs.size(), nr = (size_t)a.nr;
    if (nj == 0) return 0;
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_ml;
    const long stride = (long)e->map_local_stride;
    Span2 span;
    /* the sequences, each once */
    std::map<std::pair<const int *, size_t>, long long> at;
    long long ncode = 0;
    for (const PostLocalJob &j : jobs)
        if (at.emplace(std::make_pair(j.seq, j.L), ncode).second) ncode += (long long)j.L;
    if (e->d_ml_seq.ensure((size_t)ncode * 4 + 16)) return -1;
    for (const auto &kv : at)
        HIPCHK(hipMemcpyAsync((char *)e->d_ml_seq.p + (size_t)kv.second * 4, kv.first.first, kv.first.second * 4, hipMemcpyHostToDevice, s));
    /* the windows, in job and window order: window w of job k is job_off[k] + w */
    std::vector<ShMapLocalWin> wins;
    std::vector<size_t> job_off(nj + 1, 0), perm;
    std::map<std::pair<size_t, size_t>, MapLocalCut> cut_of;      /* (states, blocks): reads of one length share a sequence's cut */
    std::vector<const MapLocalCut *> cuts(nj, nullptr);
    std::vector<long long> seq_at(nj);
    long long scr_floats = 0;
    size_t lds = 0;
    for (size_t k = 0; k < nj; k++) {
        const PostLocalJob &j = jobs[k];
        auto found = cut_of.find(std::make_pair(j.L, j.nblock));
        if (found == cut_of.end()) {
            found = cut_of.emplace(std::make_pair(j.L, j.nblock), MapLocalCut()).first;
            (void)post_local_cut(j.L, j.nblock, nr, stride, &found->second);
        }
        cuts[k] = &found->second;
        seq_at[k] = at[std::make_pair(j.seq, j.L)];
        const size_t nw = cuts[k]->first.size();
        if (nw == 0) return set_err("map_local: nothing to cut (a sequence of %zu states, %zu blocks)", j.L, j.nblock);
        job_off[k + 1] = job_off[k] + nw;
    }
    const size_t nwin = job_off[nj];
    wins.reserve(nwin);
    for (size_t k = 0; k < nj; k++)
        for (size_t w = 0; w < cuts[k]->first.size(); w++) wins.push_back(post_local_win(jobs[k], seq_at[k], *cuts[k], w, nr, -1, scr_floats, lds));
    if (post_local_launch(e, wins, perm, lds, scr_floats, 0, 0, a, vit, tiled)) return -1;
    span.mark();
    std::vector<float> wsc(nwin);
    std::vector<int2> wend(vit ? nwin : 0);
    {
        const float *hs = d.h.as<float>();
        const int2 *he = (const int2 *)(hs + nwin);
        for (size_t k = 0; k < nwin; k++) { wsc[perm[k]] = hs[k]; if (vit) wend[perm[k]] = he[k]; }
    }
    /* per read: the highest window, the lowest on a tie; forward: sh_lse over the windows in their order */
    std::vector<size_t> bestw(nj, 0);
    for (size_t k = 0; k < nj; k++) {
        const float *sc = wsc.data() + job_off[k];
        const size_t nw = job_off[k + 1] - job_off[k];
        PostLocalJob &j = jobs[k];
        if (vit) {
            size_t b = 0;
            for (size_t w = 1; w < nw; w++) if (sc[w] > sc[b]) b = w;
            bestw[k] = b;
            j.score = sc[b];
            j.end = wend[job_off[k] + b];
            j.last = (size_t)j.end.x + 1;                    /* a path only moves right: it ends in, or left the sequence from, its highest position */
        } else {
            float acc = sc[0];
            for (size_t w = 1; w < nw; w++) acc = map_local_lse(acc, sc[w]);
            j.score = acc;
        }
    }
    if (vit && want_path) {
        /* the second pass: each read's best window alone, with its traceback; perm[k]: the job that goes k-th on the device */
        long long tb_words = 0, scr2 = 0, path_len = 0;
        size_t lds2 = 0;
        wins.clear();
        for (size_t k = 0; k < nj; k++) {
            wins.push_back(post_local_win(jobs[k], seq_at[k], *cuts[k], bestw[k], nr, tb_words, scr2, lds2));
            tb_words += (post_local_tb_words(cuts[k]->ncell[bestw[k]], jobs[k].nblock) + 3) & ~3LL;
            path_len += (long long)jobs[k].nblock;
        }
        if (post_local_launch(e, wins, perm, lds2, scr2, tb_words, path_len, a, true, tiled)) return -1;
        std::vector<long long> poff(nj);
        long long pend = 0;
        for (size_t k = 0; k < nj; k++) { poff[k] = pend; pend += (long long)jobs[perm[k]].nblock; }
        {
            const float *hs = d.h.as<float>();               /* the same window again: the same bits */
            const int2 *he = (const int2 *)(hs + nj);
            for (size_t k = 0; k < nj; k++) {
                const PostLocalJob &j = jobs[perm[k]];
                if (memcmp(&hs[k], &j.score, 4) || he[k].x != j.end.x || he[k].y != j.end.y)
                    return set_err("map_local: the second pass of a window disagrees with the first (%.9g at %d/%d, not %.9g at %d/%d)", hs[k], he[k].x, he[k].y,
                                   j.score, j.end.x, j.end.y);
            }
        }
        if (e->d_ml_lohi.ensure(nj * 8 + 16)) return -1;
        HIPCHK(hipMemcpyAsync(d.path_off.p, poff.data(), nj * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_map_local_walk, dim3((unsigned)((nj + 63) / 64)), dim3(64), 0, s, (const ShMapLocalWin *)d.rd.p, (int)nj,
                           (const unsigned *)d.tb.p, (const int2 *)d.final_state.p, (const long long *)d.path_off.p, d.paths.as<int>(),
                           e->d_ml_lohi.as<int2>());
        HIPCHK(hipGetLastError());
        int32_t *hf = (int32_t *)d.h.p, *hp = hf + 2 * nj;
        HIPCHK(hipMemcpyAsync(hf, e->d_ml_lohi.p, nj * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hp, d.paths.p, (size_t)path_len * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
        for (size_t k = 0; k < nj; k++) {
            PostLocalJob &j = jobs[perm[k]];
            j.first = (size_t)hf[2 * k];
            j.last = (size_t)hf[2 * k + 1];
            j.path = (int32_t *)malloc(j.nblock * 4);
            if (!j.path) return set_err("out of host memory");
            memcpy(j.path, hp + poff[k], j.nblock * 4);
        }
    }
    span.add(t);
    return 0;
}

/* the checks a posterior and a sequence pass before they reach the kernel; nr: posterior rows; 0 or -1 with the reason */
static int post_local_states_ok(const char *fn, size_t nr) {
    if (nr < 2) return set_err("%s: a posterior of %zu states (at least 2: one k-mer and stay)", fn, nr);
    if (nr > POST_LOCAL_MAX_STATES) return set_err("%s: a posterior of %zu states is more than the %zu a workgroup stages", fn, nr, POST_LOCAL_MAX_STATES);
    return 0;
}
static int post_local_target_ok(const char *fn, size_t nr, const int *seq, size_t L) {
    if (!seq) return set_err("%s: no sequence", fn);
    if (L == 0) return set_err("%s: an empty sequence", fn);
    if (L > MAP_LOCAL_MAX_SEQ) return set_err("%s: a sequence of %zu states is longer than the %zu a cell index holds", fn, L, MAP_LOCAL_MAX_SEQ);
    for (size_t i = 0; i < L; i++)
        if (seq[i] < 0 || (size_t)seq[i] >= nr - 1) return set_err("%s: sequence state %d at %zu is not one of the posterior's %zu k-mers", fn, seq[i], i, nr - 1);
    return 0;
}

/* ------------------------------------------------------------------ */
/* per-read symbols                                                     */
/* ------------------------------------------------------------------ */
static float post_local_one(const char *fn, const_scrappie_matrix lp, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t L, bool vit,
                            size_t *first, size_t *last, int *path) {
    if (!lp || !seq) { set_err("%s: null argument", fn); return NAN; }
    if (post_local_states_ok(fn, lp->nr)) return NAN;
    if (lp->nc == 0) { set_err("%s: a posterior of no blocks", fn); return NAN; }
    if (lp->nc > (size_t)INT32_MAX / 2) { set_err("%s: %zu blocks is too many", fn, lp->nc); return NAN; }
    if (lp->stride % 4 != 0 || lp->stride < ((lp->nr + 3) & ~(size_t)3)) { set_err("%s: a posterior whose columns are %zu floats apart (whole 16-byte pieces of %zu states)", fn, lp->stride, lp->nr); return NAN; }
    if (post_local_target_ok(fn, lp->nr, seq, L)) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    ShMapLocalArgs a{};
    a.post = post_upload_dense(e, fn, lp);
    if (!a.post) return NAN;
    a.pstride = (long long)lp->stride; a.nr = (int)lp->nr;
    a.stay_pen = stay_pen; a.skip_pen = skip_pen; a.local_pen = local_pen;
    std::vector<PostLocalJob> jobs(1);
    jobs[0].post = 0; jobs[0].lane = 0; jobs[0].nblock = lp->nc; jobs[0].seq = seq; jobs[0].L = L;
    if (post_local_run(e, jobs, a, vit, false, vit && (first || path), nullptr)) {
        free(jobs[0].path);
        (void)keep_err();
        return NAN;
    }
    if (first) *first = jobs[0].first;
    if (last) *last = jobs[0].last;
    if (path && jobs[0].path) memcpy(path, jobs[0].path, lp->nc * 4);
    free(jobs[0].path);
    return jobs[0].score;
}

extern "C" float map_to_reference_viterbi(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen, int const *seq, size_t seqlen,
                                          size_t *first, size_t *last, int *path) {
    return post_local_one("map_to_reference_viterbi", logpost, stay_pen, skip_pen, local_pen, seq, seqlen, true, first, last, path);
}
extern "C" float map_to_reference_forward(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen, int const *seq, size_t seqlen) {
    return post_local_one("map_to_reference_forward", logpost, stay_pen, skip_pen, local_pen, seq, seqlen, false, nullptr, nullptr, nullptr);
}

/* ------------------------------------------------------------------ */
/* batched                                                              */
/* ------------------------------------------------------------------ */
/* one launch group: reads idx[] of the call (post_group, sh_eng_post.inc) */
static int post_local_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const scrappie_hip_map_local_target *tg, const std::vector<size_t> &idx,
                            const scrappie_hip_params *p, bool vit, bool want_path, scrappie_hip_map_local_result *out, LaunchCut<MapLocalLoad> &cut) {
    return post_group(e, m, reads, idx, p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
        std::vector<PostLocalJob> jobs;
        for (const PostRead &q : rd) {
            PostLocalJob j;
            j.post = q.boff; j.lane = q.lane; j.nblock = q.nblock; j.seq = tg[q.r].seq; j.L = tg[q.r].seqlen;
            jobs.push_back(j);
        }
        ShMapLocalArgs a{};
        a.E = ro.E; a.sums = ro.sums; a.nr = m->NS; a.nchunk = m->ff_mtiles; a.min_prob = p->min_prob;
        a.stay_pen = p->stay_pen; a.skip_pen = p->skip_pen; a.local_pen = p->local_pen;
        const int rc = post_local_run(e, jobs, a, vit, true, vit && want_path, e->map_ms + 1);
        for (size_t k = 0; k < jobs.size(); k++) {
            if (rc) { free(jobs[k].path); continue; }
            out[rd[k].r] = scrappie_hip_map_local_result{jobs[k].score, jobs[k].nblock, jobs[k].first, jobs[k].last, jobs[k].path};
        }
        return rc;
    });
}

extern "C" int scrappie_hip_map_post_local_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_local_target *targets,
                                                 size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_local_result *out) {
    PostCall c(e, "map_post_local_batch");
    if (c.enter(!n || (reads && targets && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = scrappie_hip_map_local_result{NAN, 0, (size_t)-1, 0, nullptr};
    if (c.open(model, p, [](Model *m) {
            if (m->arch == 1) return set_err("map_post_local_batch: model '%s' is a flip-flop (CRF) model; its reads are mapped into a longer sequence with map_local_batch", m->name.c_str());
            if (post_local_states_ok("map_post_local_batch", (size_t)m->NS)) return -1;
            return ((m->NS + 3) / 4 - 1) / 4 < m->ff_mtiles ? 0 : set_err("map_post_local_batch: model '%s' has %d states in %d chunks of 16", m->name.c_str(), m->NS, m->ff_mtiles);
        })) return -1;
    Model *m = c.m;
    const bool vit = viterbi != 0, wp = want_path != 0;
    const long stride = (long)e->map_local_stride;
    const size_t nr = (size_t)m->NS;
    /* every distinct sequence of the call is checked once */
    std::map<std::pair<const int *, size_t>, std::string> checked;
    /* launch groups as scrappie_hip_map_batch cuts them; a read adds its windows, scores and scratch rows, the second pass's traceback, and its sequence
     * where no read of the group has brought it */
    LaunchCut<MapLocalLoad> cut{e, "map_post_local_batch"};
    cut.run = [&](const std::vector<size_t> &grp, MapLocalLoad &) { return post_local_group(e, m, reads, targets, grp, c.p, vit, wp, out, cut); };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        const scrappie_hip_map_local_target &t = targets[i];
        const size_t T = c.blocks(cut, i, reads[i]);
        if (T == 0) continue;
        const auto key = std::make_pair(t.seq, t.seqlen);
        auto it = checked.find(key);
        if (it == checked.end()) it = checked.emplace(key, post_local_target_ok("map_post_local_batch", nr, t.seq, t.seqlen) ? std::string(g_err) : std::string()).first;
        if (!it->second.empty()) { cut.refuse(i, it->second.c_str()); continue; }
        const size_t rb = post_local_read_bytes(t.seqlen, T, nr, stride, vit && wp), sb = t.seqlen * 4 + 16;
        c.add(cut, i, T, rb + sb,
              [&](MapLocalLoad &g, bool count) { return rb + ((count ? g.seqs.insert(key).second : !g.seqs.count(key)) ? sb : 0); },   /* (a flush clears the load: the sequence counts again) */
              "read and sequence too long for one launch group on this device");
    }
    return c.finish(cut, [&] { map_local_blank(out, n); });
}
