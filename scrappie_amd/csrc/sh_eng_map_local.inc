/* sh_eng_map_local.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * reads of a transducer model mapped INTO a longer sequence of k-mer states (k_map_local, sh_map_local.h).  The two passes -- every window of
 * every read of a launch in ONE k_map_local launch (per home), each read's best window (or their sum), with a path wanted that window again
 * with its traceback and k_map_local_walk for path, first and last -- are win_run's; the upload of the sequences, the launch group's stage
 * (the network and S1 by run_staged to STOP_POST, both passes on the posterior where S1 left it in d_E, under the engine's lock) and the
 * batch call are seq_win_run's and seq_win_batch's (all sh_eng_win.inc).  The cut of a sequence into windows is host arithmetic in sh_host.c
 * (scrappie_hip_map_local_plan).  What is here is the family's own: its form counters, its WinTraits (size formulas, planner, launch, walk),
 * the checks a posterior and a sequence pass, map_to_reference_* on the process-default engine (the caller's host posterior uploaded, the
 * dense loader) and scrappie_hip_map_post_local_batch. */

/* launches of each k_map_local form in this process: index (vit ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_map_local_forms[8];
extern "C" void scrappie_hip_map_local_form_counts(uint64_t forms[8]) {
    if (forms) for (int i = 0; i < 8; i++) forms[i] = g_map_local_forms[i].load(std::memory_order_relaxed);
}

static const size_t POST_LOCAL_MAX_STATES = (size_t)4 * SH_MAP_NTH * SH_MAPL_PIECES;      /* what a workgroup stages of a column */

template <> struct WinTraits<ShMapLocalWin> {
    using Args = ShMapLocalArgs;
    using WalkOut = int2;                                 /* first, last */
    static constexpr const char *name = "map_local";
    static constexpr size_t lds_cap = SH_MAP_LDS;
    static constexpr auto walk = k_map_local_walk;
    static DpBufs &bufs(scrappie_hip_engine *e) { return e->dp_ml; }
    static DBuf &walk_out(scrappie_hip_engine *e) { return e->d_ml_lohi; }
    static DBuf &seq_buf(scrappie_hip_engine *e) { return e->d_ml_seq; }
    static long stride(const scrappie_hip_engine *e) { return (long)e->map_local_stride; }
    static long long &at(ShMapLocalWin &r) { return r.post; }
    static size_t nr(const Args &a) { return (size_t)a.nr; }
    static size_t lds_bytes(size_t ncell, const Args &a) { return sh_map_local_lds_bytes(ncell, (size_t)a.nr); }
    static long long scr_floats(size_t ncell) { return (long long)(3 * ((ncell + 3) & ~(size_t)3)); }
    /* move codes (4 ceil(ncell / 64) words per block) and the END plane (half as many) */
    static long long tb_words(size_t ncell, size_t nblock) { return (long long)nblock * (long long)(6 * ((ncell + 63) / 64)); }
    static size_t path_len(size_t nblock) { return nblock; }
    static size_t last_of(int2 end) { return (size_t)end.x + 1; }      /* a path only moves right: it ends in, or left the sequence from, its highest position */
    static void walked(int2 w, size_t &first, size_t &last) { first = (size_t)w.x; last = (size_t)w.y; }
    static auto plan(size_t nr, long stride, size_t L, size_t nblock) {
        return [=](size_t cap, size_t *first, size_t *ncell, size_t *own, int *home, long long *scr, long long *fl) {
            return scrappie_hip_map_local_plan(L, nblock, nr, stride, cap, first, ncell, own, home, scr, fl);
        };
    }
    static size_t nc2(size_t nr, long stride, size_t L, size_t nblock) { return std::min(scrappie_hip_map_local_stride(L, nblock, nr, stride) + 2 * (nblock - 1), L); }
    static int launch(hipStream_t s, const Args &a, size_t n_lds, size_t n, size_t lds, bool vit, bool tiled) {
        return pick_bool([&](auto v, auto tl) {
                return dp_launch<k_map_local<v(), tl(), true>, k_map_local<v(), tl(), false>>(s, a, n_lds, n, SH_MAP_NTH, lds, sh_map_local_scr_lds_bytes((size_t)a.nr),
                                                                                             g_map_local_forms + ((v() ? 4 : 0) | (tl() ? 2 : 0)));
            }, vit, tiled);
    }
};

/* the checks a posterior and a sequence pass before they reach the kernel; nr: posterior rows; 0 or -1 with the reason */
static int post_local_states_ok(const char *fn, size_t nr) {
    if (nr < 2) return set_err("%s: a posterior of %zu states (at least 2: one k-mer and stay)", fn, nr);
    if (nr > POST_LOCAL_MAX_STATES) return set_err("%s: a posterior of %zu states is more than the %zu a workgroup stages", fn, nr, POST_LOCAL_MAX_STATES);
    return 0;
}
static int post_local_target_ok(const char *fn, size_t nr, const int *seq, size_t L) {
    if (!seq) return set_err("%s: no sequence", fn);
    if (L == 0) return set_err("%s: an empty sequence", fn);
    if (L > WIN_MAX_SEQ) return set_err("%s: a sequence of %zu states is longer than the %zu a cell index holds", fn, L, WIN_MAX_SEQ);
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
    return seq_win_one<ShMapLocalWin>(e, a, 0, lp->nc, seq, L, vit, first, last, path);
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
extern "C" int scrappie_hip_map_post_local_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_local_target *targets,
                                                 size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_local_result *out) {
    PostCall c(e, "map_post_local_batch");
    if (c.enter(!n || (reads && targets && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = MAP_LOCAL_NONE;
    if (c.open(model, p, [](Model *m) {
            if (m->arch == 1) return set_err("map_post_local_batch: model '%s' is a flip-flop (CRF) model; its reads are mapped into a longer sequence with map_local_batch", m->name.c_str());
            if (post_local_states_ok("map_post_local_batch", (size_t)m->NS)) return -1;
            return ((m->NS + 3) / 4 - 1) / 4 < m->ff_mtiles ? 0 : set_err("map_post_local_batch: model '%s' has %d states in %d chunks of 16", m->name.c_str(), m->NS, m->ff_mtiles);
        })) return -1;
    const Model *m = c.m;
    return seq_win_batch<ShMapLocalWin>(c, reads, targets, n, (size_t)m->NS, viterbi != 0, want_path != 0, out,
        [&](const int *seq, size_t L) { return post_local_target_ok(c.fn, (size_t)m->NS, seq, L); },
        [&](const RunOut &ro) {
            ShMapLocalArgs a{};
            a.E = ro.E; a.sums = ro.sums; a.nr = m->NS; a.nchunk = m->ff_mtiles; a.min_prob = c.p->min_prob;
            a.stay_pen = c.p->stay_pen; a.skip_pen = c.p->skip_pen; a.local_pen = c.p->local_pen;
            return a;
        });
}
