/* sh_eng_win.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * the host side that the engines which map INTO a longer reference share (k_map_crf_local, k_map_local, k_squig_local: sh_eng_map_crf_local.inc,
 * sh_eng_map_local.inc, sh_eng_squig_local.inc).  A reference is cut into windows (WinCut / win_cut / WinCuts over the family's planner in sh_host.c);
 * win_run: every window of every read of a launch in ONE launch of the family's kernel (per home; win_launch), scores and end states back, each read's
 * best window (or win_lse over its windows), and with a path wanted a second launch of that window alone with its traceback -- it must repeat the
 * first pass's bits -- the family's walk kernel and the copies; win_read_bytes: what a read adds to a launch.  A family says what is its own in a
 * WinTraits.  SeqWinJob / seq_win_run / seq_win_batch: what the two families on a launch group's posterior or transitions share beyond that -- the codes of
 * a sequence uploaded once, the launch group's stage, the batch call with its cost model. */

static const size_t WIN_MAX_SEQ = (size_t)1 << 30;      /* a cell and its kind share an int32 */

/* util.h:162-164 on the host: the windows' forward scores, in window order */
static float win_lse(float x, float y) { return fmaxf(x, y) + log1pf(expf(-fabsf(x - y))); }

/* the windows of a reference for a read, as the family's planner cuts them */
struct WinCut { std::vector<size_t> first, ncell, own; std::vector<int> home; std::vector<long long> scr; };

/* count, then fill.  plan(cap, first, ncell, own, home, scr_off, scr_floats): the family's planner of the ABI on one reference and read; returns
 * the number of windows */
template <class Plan>
static long long win_cut(Plan &&plan, WinCut *c) {
    const long long nw = plan((size_t)0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!c || nw <= 0) return nw;
    const size_t n = (size_t)nw;
    c->first.resize(n); c->ncell.resize(n); c->own.resize(n); c->home.resize(n); c->scr.resize(n);
    long long fl = 0;
    return plan(n, c->first.data(), c->ncell.data(), c->own.data(), c->home.data(), c->scr.data(), &fl);
}

/* the cuts of a launch: reads of one length (rows: blocks or samples) share a reference's cut */
struct WinCuts {
    std::map<std::pair<size_t, size_t>, WinCut> of;
    template <class Plan>
    const WinCut *get(size_t L, size_t rows, Plan &&plan) {
        auto found = of.find(std::make_pair(L, rows));
        if (found == of.end()) {
            found = of.emplace(std::make_pair(L, rows), WinCut()).first;
            (void)win_cut(plan, &found->second);
        }
        return &found->second;
    }
};

/* What a family says of its window record Rec: Args, its kernel's arguments; name, as its error texts begin; bufs(e), the DpBufs of the engine it
 * uses; lds_cap; lds_bytes(ncell, a) of a window whose rows stay in LDS, scr_floats(ncell) of one whose rows do not, tb_words(ncell, rows), the
 * entries of a read's path path_len(rows); launch(s, a, n_lds, n, lds, vit, tiled): dp_launch on its forms, its form counters and the LDS floor of
 * its scratch home; walk, its walk kernel, WalkOut, what that writes per read, into walk_out(e); last_of(end): where a path with this first-pass end
 * state ends; walked(w, first, last): first (and last, where the walk knows better) from what the walk wrote. */
template <class Rec> struct WinTraits;

/* one read of a launch as win_run sees it: its rows (blocks or samples), its reference's length, the cut of that reference for it */
struct WinJob { size_t rows, L; const WinCut *cut; };

/* one launch of the windows wins[] through the family's kernel, in device order (dp_order: those of the LDS home first; perm[k]: which of wins[] goes
 * k-th); scores and, Viterbi, end states into the DpBufs' h ([n] float, then [n] int2), which also has room for what a walk over path_len entries returns */
template <class Rec>
static int win_launch(scrappie_hip_engine *e, const std::vector<Rec> &wins, std::vector<size_t> &perm, size_t lds, long long scr_floats, long long tb_words,
                      long long path_len, typename WinTraits<Rec>::Args a, bool vit, bool tiled) {
    using T = WinTraits<Rec>;
    hipStream_t s = e->stream;
    DpBufs &d = T::bufs(e);
    const size_t n = wins.size(), n_lds = dp_order(wins, perm);
    std::vector<Rec> rd;                                  /* (one home only: wins[] is in device order already) */
    if (n_lds && n_lds < n) { rd.resize(n); for (size_t k = 0; k < n; k++) rd[k] = wins[perm[k]]; }
    if (d.ensure(n, sizeof(Rec), tb_words, scr_floats, path_len, n * (8 + 2 * sizeof(typename T::WalkOut)) + (size_t)path_len * 4 + 16, sizeof(int2))) return -1;
    HIPCHK(hipMemcpyAsync(d.rd.p, rd.empty() ? wins.data() : rd.data(), n * sizeof(Rec), hipMemcpyHostToDevice, s));
    a.rd = d.rd.as<Rec>(); a.tb = d.tb.as<unsigned>(); a.scr = d.scr.as<float>(); a.score = d.score.as<float>(); a.final_state = d.final_state.as<int2>();
    if (lds > T::lds_cap) return set_err("%s: a window of %zu bytes of LDS", T::name, lds);
    if (T::launch(s, a, n_lds, n, lds, vit, tiled)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d.h.p, d.score.p, n * 4, hipMemcpyDeviceToHost, s));
    if (vit) HIPCHK(hipMemcpyAsync((char *)d.h.p + n * 4, d.final_state.p, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    return 0;
}

/* Both passes over jobs[] (under mu, on the main stream).  a: what the kernel takes of the caller; its uploads are enqueued.  win(k, w): the record of
 * window w of job k with what is the family's own filled in; its place in the cut, its traceback and its home are filled in here.  want_path: the
 * second pass (path, first and last) on each job's best window.  Where that disagrees with the first pass, bad(k, text) decides: not 0 fails the
 * launch (the hook has set the error text), 0 leaves job k out of the walk and of give.  give(k, score, end, first, last, path) takes job k's result
 * -- first (size_t)-1 and path NULL without a second pass, path in pinned memory that the next launch overwrites -- and returns 0 or -1.
 * t (may be NULL): t[0] += from span's construction through the first pass, t[1] += the second pass, the walk and the copies. */
template <class Rec, class Win, class Bad, class Give>
static int win_run(scrappie_hip_engine *e, const std::vector<WinJob> &jobs, const typename WinTraits<Rec>::Args &a, bool vit, bool tiled, bool want_path,
                   double *t, Span2 span, Win &&win, Bad &&bad, Give &&give) {
    using T = WinTraits<Rec>;
    using Out = typename T::WalkOut;
    const size_t nj = jobs.size();
    if (nj == 0) return 0;
    hipStream_t s = e->stream;
    DpBufs &d = T::bufs(e);
    /* tb: its traceback's word offset, -1: none; scr_floats and lds take what it needs of its home */
    auto rec = [&](size_t k, size_t w, long long tb, long long &scr_floats, size_t &lds) {
        const WinCut &c = *jobs[k].cut;
        Rec r = win(k, w);
        r.first = (int)c.first[w]; r.ncell = (int)c.ncell[w]; r.own = (int)c.own[w]; r.ok = 1; r.tb = tb;
        if (c.home[w]) { r.scr = scr_floats; scr_floats += T::scr_floats(c.ncell[w]); }
        else { r.scr = -1; lds = std::max(lds, T::lds_bytes(c.ncell[w], a)); }
        return r;
    };
    /* the first pass, the windows in job and window order: window w of job k is job_off[k] + w */
    std::vector<size_t> job_off(nj + 1, 0), perm;
    for (size_t k = 0; k < nj; k++) {
        const size_t nw = jobs[k].cut->first.size();
        if (nw == 0) return set_err("%s: nothing to cut (a reference of %zu, a read of %zu)", T::name, jobs[k].L, jobs[k].rows);
        job_off[k + 1] = job_off[k] + nw;
    }
    const size_t nwin = job_off[nj];
    std::vector<Rec> wins;
    long long scr_floats = 0;
    size_t lds = 0;
    wins.reserve(nwin);
    for (size_t k = 0; k < nj; k++)
        for (size_t w = 0; w < job_off[k + 1] - job_off[k]; w++) wins.push_back(rec(k, w, -1, scr_floats, lds));
    if (win_launch(e, wins, perm, lds, scr_floats, 0, 0, a, vit, tiled)) return -1;
    span.mark();
    std::vector<float> wsc(nwin);
    std::vector<int2> wend(vit ? nwin : 0);
    {
        const float *hs = d.h.as<float>();
        const int2 *he = (const int2 *)(hs + nwin);
        for (size_t k = 0; k < nwin; k++) { wsc[perm[k]] = hs[k]; if (vit) wend[perm[k]] = he[k]; }
    }
    /* per read: the highest window, the lowest on a tie; forward: win_lse over the windows in their order */
    std::vector<size_t> bestw(nj, 0), first(nj, (size_t)-1), last(nj, 0);
    std::vector<float> score(nj);
    std::vector<int2> end(nj, make_int2(0, 0));
    std::vector<const int32_t *> path(nj, nullptr);
    std::vector<char> out(nj, 0);                         /* refused by bad() */
    for (size_t k = 0; k < nj; k++) {
        const float *sc = wsc.data() + job_off[k];
        const size_t nw = job_off[k + 1] - job_off[k];
        if (vit) {
            size_t b = 0;
            for (size_t w = 1; w < nw; w++) if (sc[w] > sc[b]) b = w;
            bestw[k] = b;
            score[k] = sc[b];
            end[k] = wend[job_off[k] + b];
            last[k] = T::last_of(end[k]);
        } else {
            float acc = sc[0];
            for (size_t w = 1; w < nw; w++) acc = win_lse(acc, sc[w]);
            score[k] = acc;
        }
    }
    if (vit && want_path) {
        /* the second pass: each read's best window alone, with its traceback; perm[k]: the job that goes k-th on the device */
        long long tb_words = 0, scr2 = 0, path_len = 0;
        size_t lds2 = 0;
        wins.clear();
        for (size_t k = 0; k < nj; k++) {
            wins.push_back(rec(k, bestw[k], tb_words, scr2, lds2));
            tb_words += (T::tb_words(jobs[k].cut->ncell[bestw[k]], jobs[k].rows) + 3) & ~3LL;      /* whole 16-byte pieces */
            path_len += (long long)T::path_len(jobs[k].rows);
        }
        if (win_launch(e, wins, perm, lds2, scr2, tb_words, path_len, a, true, tiled)) return -1;
        std::vector<long long> poff(nj);
        long long pend = 0;
        for (size_t k = 0; k < nj; k++) { poff[k] = pend; pend += (long long)T::path_len(jobs[perm[k]].rows); }
        {
            const float *hs = d.h.as<float>();               /* the same window again: the same bits */
            const int2 *he = (const int2 *)(hs + nj);
            for (size_t k = 0; k < nj; k++) {
                const size_t j = perm[k];
                if (!memcmp(&hs[k], &score[j], 4) && he[k].x == end[j].x && he[k].y == end[j].y) continue;
                char msg[240];
                snprintf(msg, sizeof msg, "the second pass of a window disagrees with the first (%.9g at %d/%d, not %.9g at %d/%d)", hs[k], he[k].x, he[k].y,
                         score[j], end[j].x, end[j].y);
                if (bad(j, msg)) return -1;
                out[j] = 1;
                poff[k] = -1;                                /* (not walked) */
            }
        }
        if (T::walk_out(e).ensure(nj * sizeof(Out) + 16)) return -1;
        HIPCHK(hipMemcpyAsync(d.path_off.p, poff.data(), nj * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(T::walk, dim3((unsigned)((nj + 63) / 64)), dim3(64), 0, s, (const Rec *)d.rd.p, (int)nj, (const unsigned *)d.tb.p,
                           (const int2 *)d.final_state.p, (const long long *)d.path_off.p, d.paths.as<int>(), T::walk_out(e).template as<Out>());
        HIPCHK(hipGetLastError());
        Out *hf = (Out *)d.h.p;
        int32_t *hp = (int32_t *)(hf + nj);
        HIPCHK(hipMemcpyAsync(hf, T::walk_out(e).p, nj * sizeof(Out), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hp, d.paths.p, (size_t)path_len * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(sh_stream_wait(s));
        for (size_t k = 0; k < nj; k++) {
            const size_t j = perm[k];
            if (out[j]) continue;
            T::walked(hf[k], first[j], last[j]);
            path[j] = hp + poff[k];
        }
    }
    for (size_t k = 0; k < nj; k++)
        if (!out[k] && give(k, score[k], end[k], first[k], last[k], path[k])) return -1;
    span.add(t);
    return 0;
}

/* device bytes one read of `rows` rows adds to a launch, its reference apart: the first pass's windows (as plan cuts them: win_cut), scores, end states and
 * scratch rows; with a path the second pass's traceback and rows on its largest window, of nc2 cells, and the path.  nwin (may be NULL): its windows. */
template <class Rec, class Plan>
static size_t win_read_bytes(Plan &&plan, size_t rows, size_t nc2, bool path, size_t *nwin = nullptr) {
    using T = WinTraits<Rec>;
    long long fl = 0;
    const long long nw = plan((size_t)0, nullptr, nullptr, nullptr, nullptr, nullptr, &fl);
    if (nwin) *nwin = (size_t)nw;
    size_t b = (size_t)nw * (sizeof(Rec) + 12) + (size_t)fl * 4 + 64;
    if (path) b += (size_t)T::tb_words(nc2, rows) * 4 + T::path_len(rows) * 4 + (size_t)T::scr_floats(nc2) * 4 + sizeof(Rec) + 64;
    return b;
}

/* ------------------------------------------------------------------ */
/* reads of a launch group into a sequence of codes (the map families)  */
/* ------------------------------------------------------------------ */
/* Beyond the above a map family's WinTraits say: at(r) -- the record's field that holds where the read's posterior or transitions begin --; seq_buf(e),
 * the DBuf of its codes; stride(e), the engine's setting; nr(a), the posterior's rows where its planner asks for them; plan(nr, stride, L, nblock),
 * its planner as win_cut takes it; nc2(nr, stride, L, nblock), the largest window of a second pass. */

/* one read of a launch: where its posterior or transitions are (as plan_add takes them), its sequence, and what comes back */
struct SeqWinJob {
    long long at; int lane; size_t nblock;
    const int *seq; size_t L;
    float score = NAN; size_t first = (size_t)-1, last = 0; int32_t *path = nullptr;
};

/* Both passes over jobs[] (under mu).  a: where the posterior or the transitions are, and what else the kernel takes of the caller.  A sequence several
 * jobs point at is uploaded once.  want_path: the second pass on each job's best window.  t (may be NULL): t[0] += the first pass, t[1] += the second
 * pass, the walk and the copies. */
template <class Rec>
static int seq_win_run(scrappie_hip_engine *e, std::vector<SeqWinJob> &jobs, typename WinTraits<Rec>::Args a, bool vit, bool tiled, bool want_path, double *t) {
    using T = WinTraits<Rec>;
    if (jobs.empty()) return 0;
    Span2 span;
    DBuf &dseq = T::seq_buf(e);
    const long stride = T::stride(e);
    /* the sequences, each once */
    std::map<std::pair<const int *, size_t>, long long> at;
    long long ncode = 0;
    for (const SeqWinJob &j : jobs)
        if (at.emplace(std::make_pair(j.seq, j.L), ncode).second) ncode += (long long)j.L;
    if (dseq.ensure((size_t)ncode * 4 + 16)) return -1;
    for (const auto &kv : at)
        HIPCHK(hipMemcpyAsync((char *)dseq.p + (size_t)kv.second * 4, kv.first.first, kv.first.second * 4, hipMemcpyHostToDevice, e->stream));
    a.seq = dseq.as<int>();
    WinCuts cuts;
    std::vector<WinJob> wj;
    std::vector<long long> seq_at;
    for (const SeqWinJob &j : jobs) {
        wj.push_back(WinJob{j.nblock, j.L, cuts.get(j.L, j.nblock, T::plan(T::nr(a), stride, j.L, j.nblock))});
        seq_at.push_back(at[std::make_pair(j.seq, j.L)]);
    }
    return win_run<Rec>(e, wj, a, vit, tiled, want_path, t, span,
        [&](size_t k, size_t) {
            const SeqWinJob &j = jobs[k];
            Rec r{};
            T::at(r) = j.at; r.lane = j.lane; r.nblock = (int)j.nblock; r.seqlen = (int)j.L; r.seq = seq_at[k];
            return r;
        },
        [&](size_t, const char *why) { return set_err("%s: %s", T::name, why); },
        [&](size_t k, float score, int2, size_t first, size_t last, const int32_t *path) {
            SeqWinJob &j = jobs[k];
            j.score = score; j.first = first; j.last = last;
            if (!path) return 0;
            j.path = (int32_t *)malloc(T::path_len(j.nblock) * 4);
            if (!j.path) return set_err("out of host memory");
            memcpy(j.path, path, T::path_len(j.nblock) * 4);
            return 0;
        });
}

/* the tail of a per-read symbol (under mu): the one read of nblock blocks that a points at, into seq; first, last and path (each may be NULL) as the
 * reference's function fills them, and its return value */
template <class Rec>
static float seq_win_one(scrappie_hip_engine *e, const typename WinTraits<Rec>::Args &a, int lane, size_t nblock, const int *seq, size_t L, bool vit,
                         size_t *first, size_t *last, int *path) {
    std::vector<SeqWinJob> jobs(1, SeqWinJob{0, lane, nblock, seq, L});
    if (seq_win_run<Rec>(e, jobs, a, vit, false, vit && (first || path), nullptr)) {
        free(jobs[0].path);
        (void)keep_err();
        return NAN;
    }
    if (first) *first = jobs[0].first;
    if (last) *last = jobs[0].last;
    if (path && jobs[0].path) memcpy(path, jobs[0].path, WinTraits<Rec>::path_len(nblock) * 4);
    free(jobs[0].path);
    return jobs[0].score;
}

/* what a launch group holds so far: MapLoad, and the sequences already counted */
struct SeqWinLoad : MapLoad { std::set<std::pair<const int *, size_t>> seqs; };

static const scrappie_hip_map_local_result MAP_LOCAL_NONE = {NAN, 0, (size_t)-1, 0, nullptr};

/* The batch call of a map family after PostCall::open: launch groups as scrappie_hip_map_batch cuts them; a read adds its windows, scores and scratch
 * rows, the second pass's traceback, and its sequence where no read of the group has brought it.  target_ok(seq, L): the family's checks of a sequence
 * (0, or -1 with the reason), made once per distinct sequence of the call; args(ro): its kernel's arguments on what the network left.  Each launch
 * group: reads idx[] of the call through post_group (sh_eng_post.inc), then seq_win_run. */
template <class Rec, class TargetOk, class MakeArgs>
static int seq_win_batch(PostCall &c, const raw_table *reads, const scrappie_hip_map_local_target *targets, size_t n, size_t nr, bool vit, bool want_path,
                         scrappie_hip_map_local_result *out, TargetOk &&target_ok, MakeArgs &&args) {
    using T = WinTraits<Rec>;
    scrappie_hip_engine *e = c.e;
    const long stride = T::stride(e);
    std::map<std::pair<const int *, size_t>, std::string> checked;
    LaunchCut<SeqWinLoad> cut{e, c.fn};
    cut.run = [&](const std::vector<size_t> &grp, SeqWinLoad &) {
        return post_group(e, c.m, reads, grp, c.p, cut, [&](const RunOut &ro, const std::vector<PostRead> &rd) {
            std::vector<SeqWinJob> jobs;
            for (const PostRead &q : rd) jobs.push_back(SeqWinJob{q.boff, q.lane, q.nblock, targets[q.r].seq, targets[q.r].seqlen});
            const int rc = seq_win_run<Rec>(e, jobs, args(ro), vit, true, vit && want_path, e->map_ms + 1);
            for (size_t k = 0; k < jobs.size(); k++) {
                if (rc) { free(jobs[k].path); continue; }
                out[rd[k].r] = scrappie_hip_map_local_result{jobs[k].score, jobs[k].nblock, jobs[k].first, jobs[k].last, jobs[k].path};
            }
            return rc;
        });
    };
    for (size_t i = 0; i < n && !cut.failed; i++) {
        const scrappie_hip_map_local_target &t = targets[i];
        const size_t nb = c.blocks(cut, i, reads[i]);
        if (nb == 0) continue;
        const auto key = std::make_pair(t.seq, t.seqlen);
        auto it = checked.find(key);
        if (it == checked.end()) it = checked.emplace(key, target_ok(t.seq, t.seqlen) ? std::string(g_err) : std::string()).first;
        if (!it->second.empty()) { cut.refuse(i, it->second.c_str()); continue; }
        const size_t rb = win_read_bytes<Rec>(T::plan(nr, stride, t.seqlen, nb), nb, T::nc2(nr, stride, t.seqlen, nb), vit && want_path), sb = t.seqlen * 4 + 16;
        c.add(cut, i, nb, rb + sb,
              [&](SeqWinLoad &g, bool count) { return rb + ((count ? g.seqs.insert(key).second : !g.seqs.count(key)) ? sb : 0); },   /* (a flush clears the load: the sequence counts again) */
              "read and sequence too long for one launch group on this device");
    }
    return c.finish(cut, [&] { for (size_t i = 0; i < n; i++) { free(out[i].path); out[i] = MAP_LOCAL_NONE; } });
}
