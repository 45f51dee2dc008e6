/* sh_eng_post.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * the host side that the engines on a launch group's resident posterior or transitions share (k_map, k_map_crf, k_map_pack, k_map_crf_pack,
 * k_map_crf_local, k_crf_find: sh_eng_map*.inc, sh_eng_crf_find.inc).  Per-read plumbing (Span2, post_upload_*, the base-code check, best_finite); DpPlan /
 * plan_add / dp_run: per-read records through a kernel with two homes, over a family's DpTraits; PackSet / PackSets / PackLaunch: sets of short
 * sequences packed into workgroups; PostCall: the batch call (preamble, memory model, the refusals of a read's length, the load of a launch group);
 * post_group: the network of a launch group to STOP_POST under the engine's lock, then the family's launches.  A family file keeps what is its own:
 * record layout, size formulas, the kernel launch, its result handling. */

/* ------------------------------------------------------------------ */
/* per-read plumbing                                                    */
/* ------------------------------------------------------------------ */
/* two spans of host time: from construction to mark(), from mark() to add(t), which adds them to t[0] and t[1] (t may be NULL) */
struct Span2 {
    using Clock = std::chrono::steady_clock;
    Clock::time_point t0 = Clock::now(), t1 = t0;
    void mark() { t1 = Clock::now(); }
    void add(double *t) const {
        if (!t) return;
        t[0] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t[1] += std::chrono::duration<double, std::milli>(Clock::now() - t1).count();
    }
};

/* a per-read call's host matrix into d_map_post, on the main stream (under mu); where it is on the device, NULL with the reason */
static const float *post_upload(scrappie_hip_engine *e, const char *fn, const float *src, size_t nfloat) {
    DBuf &d = e->d_map_post;
    if (d.ensure(nfloat * 4)) return nullptr;
    if (hipMemcpyAsync(d.p, src, nfloat * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess) { set_err("%s: upload failed", fn); return nullptr; }
    return d.as<float>();
}
static const float *post_upload_dense(scrappie_hip_engine *e, const char *fn, const_scrappie_matrix lp) {
    return post_upload(e, fn, lp->data.f, lp->nc * lp->stride);
}
/* a transition matrix of 25 rows: as far as the last column's 25th float */
static const float *post_upload_trans(scrappie_hip_engine *e, const char *fn, const_scrappie_matrix tr) {
    return post_upload(e, fn, tr->data.f, (tr->nc - 1) * tr->stride + 25);
}

/* base codes: where the first of seq[0..L) that is none stands (L: all are), and what to say of it */
static size_t first_non_base(const int *seq, size_t L) {
    size_t i = 0;
    while (i < L && seq[i] >= 0 && seq[i] <= 3) i++;
    return i;
}
static std::string non_base_text(const int *seq, size_t i) {
    return "sequence code " + std::to_string(seq[i]) + " at " + std::to_string(i) + " is not a base (0..3)";
}
static int bases_ok(const char *fn, const int *seq, size_t L) {
    const size_t i = first_non_base(seq, L);
    return i < L ? set_err("%s: %s", fn, non_base_text(seq, i).c_str()) : 0;
}

/* the highest finite score, the lowest index on a tie; -1: none */
static int best_finite(const float *score, size_t n) {
    int best = -1;
    for (size_t k = 0; k < n; k++)
        if (std::isfinite(score[k]) && (best < 0 || score[k] > score[best])) best = (int)k;
    return best;
}

/* ------------------------------------------------------------------ */
/* one plan and one runner for a kernel with two homes                  */
/* ------------------------------------------------------------------ */
/* What a family says of its record type Rec: Args, its kernel's arguments; at(r) -- the field that holds where the read's posterior or transitions
 * begin --; lds_bytes(L) of a read whose rows stay in LDS, scr_floats(L) of one whose rows do not, tb_words(L, nblock), the entries of a path and
 * of a band edge, path_len(nblock) and band_len(nblock); launch(s, a, n_lds, n, lds, vit, band, tiled): dp_launch on its forms; walk, its walk
 * kernel; none(score): the kernel found no admissible path (the score becomes NAN, the path stays away). */
template <class Rec> struct DpTraits;

/* host side of one launch: the reads' records, their codes and bands laid end to end, traceback / scratch offsets */
template <class Rec>
struct DpPlan {
    std::vector<Rec> rd;
    std::vector<int> seq, band;
    std::vector<long long> path_off;      /* per read, -1: no path */
    long long tb_words = 0, scr_floats = 0, path_len = 0;
    size_t lds = 0;
};

template <class Rec>
static void plan_add(DpPlan<Rec> &pl, long long at, int lane, size_t nblock, const int *seq, size_t L, const size_t *lo, const size_t *hi, bool path) {
    using T = DpTraits<Rec>;
    Rec r{};
    T::at(r) = at; r.lane = lane; r.nblock = (int)nblock; r.seqlen = (int)L; r.ok = 1;
    r.seq = (long long)pl.seq.size();
    pl.seq.insert(pl.seq.end(), seq, seq + L);
    r.band = -1;
    if (lo) {
        r.band = (long long)pl.band.size();
        for (size_t i = 0; i < T::band_len(nblock); i++) pl.band.push_back((int)lo[i]);
        for (size_t i = 0; i < T::band_len(nblock); i++) pl.band.push_back((int)hi[i]);
    }
    r.tb = -1;
    if (path) {
        r.tb = pl.tb_words; pl.tb_words += T::tb_words(L, nblock);
        pl.path_off.push_back(pl.path_len); pl.path_len += (long long)T::path_len(nblock);
    } else pl.path_off.push_back(-1);
    if (T::lds_bytes(L) <= SH_MAP_LDS) { r.scr = -1; pl.lds = std::max(pl.lds, T::lds_bytes(L)); }
    else { r.scr = pl.scr_floats; pl.scr_floats += T::scr_floats(L); }
    pl.rd.push_back(r);
}

/* The scratch part of the plan plan_add makes of reads of seqlen[i] codes and nblock[i] blocks, in this order in one launch (no traceback, no bands):
 * off[i] = the float offset of read i's score rows in the scratch allocation, -1 where they live in LDS; returns the floats the launch allocates for
 * them all.  Host arithmetic only: behind the planning symbols of the ABI. */
template <class Rec>
static long long plan_scratch(const size_t *seqlen, const size_t *nblock, size_t n, long long *off) {
    DpPlan<Rec> pl;
    std::vector<int> codes;
    for (size_t i = 0; i < n; i++) {
        codes.assign(seqlen[i], 0);
        plan_add(pl, 0, 0, nblock[i], codes.data(), seqlen[i], nullptr, nullptr, false);
        if (off) off[i] = pl.rd[i].scr;
    }
    return pl.scr_floats;
}

/* One plan (for k_map all banded or all unbanded) through its kernel and its walk (under mu, on the main stream, in dp_map): the records staged in
 * device order (dp_order), codes, bands and path offsets uploaded, the family's launch, dp_collect; scores into score[], paths into paths[i]
 * (malloc'd, only where the plan holds a path and one exists; paths may be NULL).  a: where the posterior or the transitions are, and what else the
 * kernel takes of the caller.  t (may be NULL): t[0] += the kernel, t[1] += walk + copies. */
template <class Rec>
static int dp_run(scrappie_hip_engine *e, DpPlan<Rec> &pl, typename DpTraits<Rec>::Args a, bool vit, bool band, bool tiled, float *score, int32_t **paths,
                  double *t) {
    using T = DpTraits<Rec>;
    const size_t n = pl.rd.size();
    if (n == 0) return 0;
    hipStream_t s = e->stream;
    DpBufs &d = e->dp_map;
    std::vector<size_t> perm;
    const size_t n_lds = dp_order(pl.rd, perm);
    std::vector<Rec> rd(n);
    std::vector<long long> poff(n);
    for (size_t k = 0; k < n; k++) { rd[k] = pl.rd[perm[k]]; poff[k] = pl.path_off[perm[k]]; }
    if (d.ensure(n, sizeof(Rec), pl.tb_words, pl.scr_floats, pl.path_len) || e->d_map_seq.ensure(pl.seq.size() * 4 + 16) ||
        e->d_map_band.ensure(pl.band.size() * 4 + 16)) return -1;
    HIPCHK(hipMemcpyAsync(d.rd.p, rd.data(), n * sizeof(Rec), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_map_seq.p, pl.seq.data(), pl.seq.size() * 4, hipMemcpyHostToDevice, s));
    if (!pl.band.empty()) HIPCHK(hipMemcpyAsync(e->d_map_band.p, pl.band.data(), pl.band.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.path_off.p, poff.data(), n * 8, hipMemcpyHostToDevice, s));
    a.rd = d.rd.as<Rec>(); a.seq = e->d_map_seq.as<int>(); a.band = e->d_map_band.as<int>(); a.tb = d.tb.as<unsigned>(); a.scr = d.scr.as<float>();
    a.score = d.score.as<float>(); a.final_state = d.final_state.as<int>();
    Span2 span;
    if (T::launch(s, a, n_lds, n, pl.lds, vit, band, tiled)) return -1;
    HIPCHK(hipGetLastError());
    HIPCHK(sh_stream_wait(s));
    span.mark();
    if (dp_collect<T::walk, Rec>(s, d, perm, pl.path_off, pl.path_len, vit && !band && pl.path_len > 0, [&](size_t i, float sc, const int32_t *p) {
            const bool none = T::none(sc);
            score[i] = none ? NAN : sc;
            if (!paths) return 0;
            paths[i] = nullptr;
            if (!p || none) return 0;
            const size_t ne = T::path_len((size_t)pl.rd[i].nblock);
            paths[i] = (int32_t *)malloc(ne * 4);
            if (!paths[i]) return set_err("out of host memory");
            memcpy(paths[i], p, ne * 4);
            return 0;
        })) return -1;
    span.add(t);
    return 0;
}

/* ------------------------------------------------------------------ */
/* sets of short sequences packed into workgroups                       */
/* ------------------------------------------------------------------ */
/* One cand array of a call as every read that points at it sees it: checked, packed and laid out as its kernel reads it, once.  A family derives
 * its set from this and fills it (how a candidate or motif becomes cell words is its own).  PackSet: of block-mapping targets. */
struct PackSpan { size_t cell, first, at, ncell, nitem; };       /* where a pack's cell words, its first cells and its members begin in cellw / firsts / packed */
template <class Target_>
struct PackSetOf {
    using Target = Target_;
    using Pack = PackSpan;
    const Target *cand = nullptr;
    size_t n = 0;
    std::string why;                          /* why its first member that cannot be run cannot */
    std::vector<Pack> packs;
    std::vector<int> cellw, firsts;           /* (firsts: k_map_pack's alone) */
    std::vector<size_t> packed;               /* the members in pack order */
    size_t bytes = 0;                         /* device bytes a read of this set adds to a launch */
};
using PackSet = PackSetOf<scrappie_hip_map_target>;

/* the sets of a call, one per distinct (cand, n), built on first sight; of[i]: read i's */
template <class Set>
struct PackSets {
    std::map<std::pair<const typename Set::Target *, size_t>, std::unique_ptr<Set>> sets;
    std::vector<const Set *> of;
    template <class Build>
    const Set *get(const typename Set::Target *cand, size_t n, Build &&build) {
        std::unique_ptr<Set> &cs = sets[std::make_pair(cand, n)];
        if (!cs) { cs.reset(new Set()); build(*cs); }
        return cs.get();
    }
};

/* One launch over jobs[] (each with a set, cs): the sets' tables end to end, a set's once however many jobs point at it, and the jobs' scores end to
 * end in job and pack order -- out0[j]: where job j's begin.  lay() calls emit(j, P, cell0, first0, out) for every pack P of every job: where its
 * set's cell words and first cells begin in cellw / firsts, and where its scores go.  scatter() calls put(job, k, slot) for every packed member k. */
template <class Set>
struct PackLaunch {
    std::vector<int> cellw, firsts;
    std::map<const Set *, std::pair<size_t, size_t>> up;
    std::vector<size_t> out0;
    size_t nscore = 0;
    template <class Jobs, class Emit>
    void lay(const Jobs &jobs, Emit &&emit) {
        out0.assign(jobs.size(), 0);
        for (size_t j = 0; j < jobs.size(); j++) {
            const Set &cs = *jobs[j].cs;
            out0[j] = nscore;
            if (cs.packs.empty()) continue;
            auto it = up.find(&cs);
            if (it == up.end()) {
                it = up.emplace(&cs, std::make_pair(cellw.size(), firsts.size())).first;
                cellw.insert(cellw.end(), cs.cellw.begin(), cs.cellw.end());
                firsts.insert(firsts.end(), cs.firsts.begin(), cs.firsts.end());
            }
            for (const PackSet::Pack &P : cs.packs) emit(j, P, it->second.first + P.cell, it->second.second + P.first, nscore + P.at);
            nscore += cs.packed.size();
        }
    }
    template <class Jobs, class Put>
    void scatter(Jobs &jobs, Put &&put) const {
        for (size_t j = 0; j < jobs.size(); j++) {
            const Set &cs = *jobs[j].cs;
            for (size_t i = 0; i < cs.packed.size(); i++) put(jobs[j], cs.packed[i], out0[j] + i);
        }
    }
};

/* ------------------------------------------------------------------ */
/* the batch call and its launch groups                                 */
/* ------------------------------------------------------------------ */
static size_t map_read_nsample(const Model *m, const raw_table &rt) {
    const size_t nf = (rt.raw && rt.end > rt.start) ? rt.end - rt.start : 0;
    return m->arch == 3 ? nf / (size_t)m->nfeat : nf;            /* events: raw holds [nevent][12] features */
}
static size_t map_blocks(const Model *m, size_t ns) {
    return ns >= m->min_samples ? (ns + (size_t)m->stride - 1) / (size_t)m->stride : 0;       /* build_group */
}

/* what a launch group holds so far, as its cost counts it (a family may derive from it what else it counts once per group) */
struct MapLoad { size_t sumT = 0, maxT = 0, extra = 0; };

/* A batch call of a family: enter() (the null check, one call at a time inside the engine), the family blanks its out[], open() (the model, the
 * family's check of it, the default parameters, the device, map_ms zeroed, the memory model), then per read in input order blocks() and add() on the
 * family's LaunchCut, and finish().  Launch groups are bounded by reads and by device memory: the materialised posterior and the arena of the
 * network (bytes_per_block with the posterior: ~66 KB per column block of 16 reads for 4^5 + 1 states), plus what each read adds of its own. */
struct PostCall {
    scrappie_hip_engine *e;
    const char *fn;                   /* the batch function's name, as its error texts begin */
    std::unique_lock<std::mutex> call;
    Model *m = nullptr;
    scrappie_hip_params dp;
    const scrappie_hip_params *p = nullptr;
    size_t bpb = 0, budget = 0;
    PostCall(scrappie_hip_engine *e_, const char *fn_) : e(e_), fn(fn_) {}
    PostCall(const PostCall &) = delete;
    int enter(bool args_ok) {
        if (!e || !args_ok) return set_err("%s: null argument", fn);
        call = std::unique_lock<std::mutex>(e->call_mu);
        return 0;
    }
    template <class ModelOk>
    int open(int model, const scrappie_hip_params *params, ModelOk &&model_ok) {
        m = get_model(e, model);
        if (!m || model_ok(m)) return -1;
        dp = scrappie_hip_default_params();
        p = params ? params : &dp;
        (void)hipSetDevice(e->device);
        for (double &x : e->map_ms) x = 0.0;
        bpb = bytes_per_block(m, true);
        budget = e->max_launch_blocks ? e->max_launch_blocks * bpb : (size_t)(e->mem_frac * (double)e->total_mem);
        return 0;
    }
    size_t cost(size_t sumT, size_t maxT, size_t extra) const { return (sumT / 16 + maxT + 1) * bpb + extra; }
    /* the blocks of read i; 0: refused */
    template <class Cut>
    size_t blocks(Cut &cut, size_t i, const raw_table &read) const {
        const size_t T = map_blocks(m, map_read_nsample(m, read));
        if (T == 0) cut.refuse(i, "read too short for the model (or empty)");
        else if (T > (size_t)INT32_MAX / 2) cut.refuse(i, "too many blocks");
        else return T;
        return 0;
    }
    /* read i of T blocks into the cut: refused with too_long where it fits no launch group alone (alone: its own bytes); else extra(load, false) is
     * what it would add to the group as it stands and extra(load, true), after the cut has made room, counts it in */
    template <class Cut, class Extra>
    void add(Cut &cut, size_t i, size_t T, size_t alone, Extra &&extra, const char *too_long) const {
        if (cost(T, T, alone) > budget) { cut.refuse(i, too_long); return; }
        const auto &g = cut.load;
        cut.add(i, cut.who.size() < e->max_launch_reads && cost(g.sumT + T, std::max(g.maxT, T), g.extra + extra(cut.load, false)) <= budget);
        auto &h = cut.load;                                        /* (a flush has cleared it) */
        h.sumT += T; h.maxT = std::max(h.maxT, T); h.extra += extra(h, true);
    }
    template <class Cut>
    void add(Cut &cut, size_t i, size_t T, size_t bytes, const char *too_long) const {
        add(cut, i, T, bytes, [bytes](const auto &, bool) { return bytes; }, too_long);
    }
    template <class Cut, class Blank>
    int finish(Cut &cut, Blank &&blank) const {
        return cut.finish(blank, [this](size_t i, const char *why) { set_err("%s: read %zu: %s", fn, i, why); });
    }
};

/* one read of a launch group after the network: which read of the call, and where its posterior or transitions lie (first column block, lane) */
struct PostRead { size_t r; long long boff; int lane; size_t nblock; };

/* One launch group: reads idx[] of the call through the network to STOP_POST, under the engine's lock; the reads whose signal is out of range are
 * refused through the cut; body(ro, rd) -- the family's launches on what the network left in d_E -- runs with the lock still held: d_E is the
 * engine's, and the next group overwrites it. */
template <class Cut, class Body>
static int post_group(scrappie_hip_engine *e, Model *m, const raw_table *reads, const std::vector<size_t> &idx, const scrappie_hip_params *p, Cut &cut,
                      Body &&body) {
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const raw_table *> win;
    win.reserve(idx.size());
    for (size_t r : idx) win.push_back(&reads[r]);
    RunOut ro;
    std::vector<unsigned> bad;
    if (run_staged(e, m, win, p, STOP_POST, 5, &ro, bad, e->map_ms)) return -1;
    const LaunchGroup &lg = e->current().lg;
    std::vector<PostRead> rd;
    rd.reserve(idx.size());
    for (size_t i = 0; i < lg.npad; i++) {
        const int o = lg.order[i];
        if (o < 0 || lg.rT[i] <= 0) continue;
        const size_t r = idx[(size_t)o];
        if (bad[i]) cut.refuse(r, "the read holds values outside the supported range (is the signal trimmed and med/MAD-normalised?)");
        else rd.push_back(PostRead{r, lg.tile_boff[i >> 4], (int)(i & 15), (size_t)lg.rT[i]});
    }
    return body(ro, rd);
}
