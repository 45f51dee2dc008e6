/* sh_eng_cut.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * what the batched engines beside the basecaller share (sh_eng_map*.inc, sh_eng_crf_find.inc, sh_eng_squig.inc, sh_eng_sqnet.inc, sh_eng_events.inc;
 * sh_eng_post.inc builds on it what the engines on a resident posterior share further).  keep_err: the way out of a failed launch.  LaunchCut: a call cut into launches
 * that fit the device, in input order, with the first refusal remembered and one way out of a failed launch.  dp_order / dp_launch / dp_collect: the
 * per-read DP records of k_map and k_squig through a kernel with two homes (score rows in LDS, or in device scratch for the reads too long for it). */

/* what one launch may hold: half of the device memory that is free now (the engine's own arena stays where it is), a quarter of all of it where the
 * runtime will not say; override: the bytes a debug option has set */
/* the way out of a failed launch: HIP's sticky error cleared, the error text as it was before that; -1 */
static int keep_err() {
    const std::string keep = g_err;
    (void)hipGetLastError();
    return set_err("%s", keep.c_str());
}

static size_t launch_budget(const scrappie_hip_engine *e, size_t override) {
    if (override) return override;
    size_t fr = 0, tot = 0;
    return hipMemGetInfo(&fr, &tot) == hipSuccess ? fr / 2 : e->total_mem / 4;
}

/* A batch function walks its items in input order (`for (i = 0; i < n && !cut.failed; i++)`): refuse(i, why) for an item that reaches no launch (its
 * own checks; one that cannot fit a launch alone), add(i, fits) for the others -- fits: would the launch still be within the device and the count caps
 * WITH this item (the caller's cost model over `load`, which it adds the item to afterwards; the cost need not be additive) -- and finish().
 * run(who, load) is one launch over the members who[]; it may refuse members too (what only the device finds out).  A failed launch -- a HIP error, or
 * the debug option fail_run counting down to this launch, which then is refused here, on the host, before anything is uploaded -- ends the call: its
 * error text is kept, HIP's sticky error cleared and the streams waited for (only them: the squiggle engines do not hold call_mu, and drain() would
 * clear the slots' pending flags under a deferred call), so the engine stays usable. */
template <class Load>
struct LaunchCut {
    scrappie_hip_engine *e;
    const char *fn;                   /* the batch function's name, as its error texts begin */
    std::function<int(const std::vector<size_t> &, Load &)> run;
    std::vector<size_t> who;          /* the launch being assembled: indices into the call, in input order */
    Load load{};                      /* what the caller's cost model has summed over who[]; cleared with it */
    size_t bad = (size_t)-1;          /* the first refusal in input order */
    std::string why;
    bool failed = false;
    void refuse(size_t i, const char *text) { if (i < bad) { bad = i; why = text; } }
    void flush() {
        if (who.empty() || failed) return;
        if ((e->dbg_fail_run > 0 && --e->dbg_fail_run == 0) ? set_err("%s: injected failure (debug option fail_run)", fn) : run(who, load)) {
            failed = true;
            (void)keep_err();
            (void)sh_stream_wait(e->pstream); (void)sh_stream_wait(e->stream); (void)sh_stream_wait(e->cstream);
        }
        who.clear(); load = Load{};
    }
    void add(size_t i, bool fits) {
        if (!fits) flush();
        who.push_back(i);
    }
    /* the last launch, then the call's answer: -1 after a failed launch (blank() has freed and emptied out[]), else 0 with the first refusal -- if any, as
     * say(index, reason) words it -- as the error text */
    template <class Blank, class Say>
    int finish(Blank &&blank, Say &&say) {
        flush();
        if (failed) { blank(); return -1; }
        if (bad != (size_t)-1) say(bad, why.c_str());
        return 0;
    }
};

static void timing3(const double *ms, double out[3]) {
    for (int k = 0; k < 3; k++) out[k] = ms ? ms[k] : 0.0;
}
template <class Res>
static void free_paths(Res *r, size_t n) {
    if (!r) return;
    for (size_t i = 0; i < n; i++) { free(r[i].path); r[i].path = nullptr; }
}

/* ------------------------------------------------------------------ */
/* per-read DP records through a kernel with two homes (DpBufs)         */
/* ------------------------------------------------------------------ */
/* device order: the records whose rows fit LDS first (one launch), then those in scratch (another); perm[k]: which record of the plan goes k-th;
 * returns how many are of the first kind */
template <class Rec>
static size_t dp_order(const std::vector<Rec> &rd, std::vector<size_t> &perm) {
    perm.resize(rd.size());
    std::iota(perm.begin(), perm.end(), (size_t)0);
    return (size_t)(std::stable_partition(perm.begin(), perm.end(), [&](size_t i) { return rd[i].scr < 0; }) - perm.begin());
}

/* one workgroup of nth threads per record: K_LDS over the first n_lds records with lds bytes of dynamic LDS, K_SCR over the rest with scr_lds;
 * forms[0] / forms[1] count the launches of either; 0, or -1 as launch_k says */
template <auto K_LDS, auto K_SCR, class Args>
static int dp_launch(hipStream_t s, const Args &a, size_t n_lds, size_t n, unsigned nth, size_t lds, size_t scr_lds, std::atomic<uint64_t> *forms) {
    if (n_lds) {
        forms[0].fetch_add(1, std::memory_order_relaxed);
        if (launch_k<K_LDS>(dim3((unsigned)n_lds), dim3(nth), lds, s, a)) return -1;
    }
    if (n > n_lds) {                     /* the reads whose rows live in scratch: the records' tail */
        Args b = a;
        b.rd += n_lds; b.score += n_lds; b.final_state += n_lds;
        forms[1].fetch_add(1, std::memory_order_relaxed);
        if (launch_k<K_SCR>(dim3((unsigned)(n - n_lds)), dim3(nth), scr_lds, s, b)) return -1;
    }
    return 0;
}

/* after the kernel: K_WALK (one thread per record) where paths are wanted, scores and paths to the host, and give(i, score, path) for every record in
 * the plan's order -- path: the record's slice of the walked paths (path_off[i], the plan's), nullptr where it has none; give returns 0 or -1 */
template <auto K_WALK, class Rec, class Give>
static int dp_collect(hipStream_t s, DpBufs &d, const std::vector<size_t> &perm, const std::vector<long long> &path_off, long long path_len, bool walk,
                      Give &&give) {
    const size_t n = perm.size();
    if (walk) {
        hipLaunchKernelGGL(K_WALK, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const Rec *)d.rd.p, (int)n, (const unsigned *)d.tb.p,
                           (const int *)d.final_state.p, (const long long *)d.path_off.p, d.paths.as<int>());
        HIPCHK(hipGetLastError());
    }
    float *hs = d.h.as<float>();
    int32_t *hp = (int32_t *)(hs + n);
    HIPCHK(hipMemcpyAsync(hs, d.score.p, n * 4, hipMemcpyDeviceToHost, s));
    if (walk) HIPCHK(hipMemcpyAsync(hp, d.paths.p, (size_t)path_len * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(sh_stream_wait(s));
    for (size_t k = 0; k < n; k++) {
        const size_t i = perm[k];
        if (give(i, hs[k], walk && path_off[i] >= 0 ? hp + path_off[i] : nullptr)) return -1;
    }
    return 0;
}
