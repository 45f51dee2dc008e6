/* sh_eng_map_crf_local.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * reads of a flip-flop (CRF) model mapped INTO a longer base sequence (k_map_crf_local, sh_map_crf_local.h).  The two passes -- every window of
 * every read of a launch in ONE k_map_crf_local launch (per home), each read's best window (or their sum), with a path wanted that window again
 * with its traceback and k_map_crf_local_walk for path and first -- are win_run's; the upload of the sequences, the launch group's stage
 * (run_staged to STOP_POST, both passes on the transitions where k_crf left them in d_E, under the engine's lock) and the batch call are
 * seq_win_run's and seq_win_batch's (all sh_eng_win.inc).  The cut of a sequence into windows is host arithmetic in sh_host.c
 * (scrappie_hip_map_crf_local_plan).  What is here is the family's own: its form counters, its WinTraits (size formulas, planner, launch, walk),
 * the checks a sequence passes, map_crf_to_reference_* on the process-default engine (the caller's host matrix uploaded, the reference-layout
 * loader) and scrappie_hip_map_local_batch. */

/* launches of each k_map_crf_local form in this process: index (vit ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
static std::atomic<uint64_t> g_map_crf_local_forms[8];
extern "C" void scrappie_hip_map_crf_local_form_counts(uint64_t forms[8]) {
    if (forms) for (int i = 0; i < 8; i++) forms[i] = g_map_crf_local_forms[i].load(std::memory_order_relaxed);
}

template <> struct WinTraits<ShMapCrfLocalWin> {
    using Args = ShMapCrfLocalArgs;
    using WalkOut = int;                                  /* first; last is the end cell */
    static constexpr const char *name = "map_crf_local";
    static constexpr size_t lds_cap = SH_MAP_LDS;
    static constexpr auto walk = k_map_crf_local_walk;
    static DpBufs &bufs(scrappie_hip_engine *e) { return e->dp_mcl; }
    static DBuf &walk_out(scrappie_hip_engine *e) { return e->d_mcl_first; }
    static DBuf &seq_buf(scrappie_hip_engine *e) { return e->d_mcl_seq; }
    static long stride(const scrappie_hip_engine *e) { return (long)e->map_crf_local_stride; }
    static long long &at(ShMapCrfLocalWin &r) { return r.trans; }
    static size_t nr(const Args &) { return 0; }
    static size_t lds_bytes(size_t ncell, const Args &) { return sh_map_crf_local_lds_bytes(ncell); }
    static long long scr_floats(size_t ncell) { return (long long)(4 * (ncell + 1)); }
    static long long tb_words(size_t ncell, size_t nblock) { return (long long)nblock * (long long)(4 * ((ncell + 63) / 64)); }
    static size_t path_len(size_t nblock) { return nblock + 1; }
    static size_t last_of(int2 end) { return (size_t)end.x; }
    static void walked(int w, size_t &first, size_t &) { first = (size_t)w; }
    static auto plan(size_t, long stride, size_t L, size_t nblock) {
        return [=](size_t cap, size_t *first, size_t *ncell, size_t *own, int *home, long long *scr, long long *fl) {
            return scrappie_hip_map_crf_local_plan(L, nblock, stride, cap, first, ncell, own, home, scr, fl);
        };
    }
    static size_t nc2(size_t, long stride, size_t L, size_t nblock) { return std::min(scrappie_hip_map_crf_local_stride(L, nblock, stride) + nblock, L + 1); }
    static int launch(hipStream_t s, const Args &a, size_t n_lds, size_t n, size_t lds, bool vit, bool tiled) {
        return pick_bool([&](auto v, auto tl) {
                using LD = std::conditional_t<tl(), ShCrfTiled, ShCrfRef>;
                return dp_launch<k_map_crf_local<v(), LD, true>, k_map_crf_local<v(), LD, false>>(s, a, n_lds, n, SH_MAP_NTH, lds, SH_MAPC_HEAD * 4,
                                                                                                 g_map_crf_local_forms + ((v() ? 4 : 0) | (tl() ? 2 : 0)));
            }, vit, tiled);
    }
};

/* the checks a sequence passes before it reaches the kernel; 0 or -1 with the reason */
static int map_local_target_ok(const char *fn, const int *seq, size_t L) {
    if (!seq) return set_err("%s: no sequence", fn);
    if (L == 0) return set_err("%s: an empty sequence", fn);
    if (L > WIN_MAX_SEQ) return set_err("%s: a sequence of %zu bases is longer than the %zu a cell index holds", fn, L, WIN_MAX_SEQ);
    return bases_ok(fn, seq, L);
}

/* ------------------------------------------------------------------ */
/* per-read symbols                                                     */
/* ------------------------------------------------------------------ */
static float map_local_one(const char *fn, const_scrappie_matrix tr, const int *seq, size_t L, bool vit, size_t *first, size_t *last, int *path) {
    if (!tr || !seq) { set_err("%s: null argument", fn); return NAN; }
    if (!sh_crf_post_ok(tr)) { set_err("%s: not a transition matrix of 25 rows and at least one block", fn); return NAN; }
    if (tr->nc > (size_t)INT32_MAX / 2) { set_err("%s: %zu blocks is too many", fn, tr->nc); return NAN; }
    if (map_local_target_ok(fn, seq, L)) return NAN;
    scrappie_hip_engine *e = default_engine();
    if (!e) return NAN;
    (void)hipSetDevice(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    ShMapCrfLocalArgs a{};
    a.trans = post_upload_trans(e, fn, tr);
    if (!a.trans) return NAN;
    return seq_win_one<ShMapCrfLocalWin>(e, a, (int)tr->stride, tr->nc, seq, L, vit, first, last, path);
}

extern "C" float map_crf_to_reference_viterbi(const_scrappie_matrix trans, int const *seq, size_t seqlen, size_t *first, size_t *last, int *path) {
    return map_local_one("map_crf_to_reference_viterbi", trans, seq, seqlen, true, first, last, path);
}
extern "C" float map_crf_to_reference_forward(const_scrappie_matrix trans, int const *seq, size_t seqlen) {
    return map_local_one("map_crf_to_reference_forward", trans, seq, seqlen, false, nullptr, nullptr, nullptr);
}

/* ------------------------------------------------------------------ */
/* batched                                                              */
/* ------------------------------------------------------------------ */
extern "C" void scrappie_hip_free_map_local_results(scrappie_hip_map_local_result *r, size_t n) { free_paths(r, n); }

extern "C" int scrappie_hip_map_local_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_local_target *targets,
                                            size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_local_result *out) {
    PostCall c(e, "map_local_batch");
    if (c.enter(!n || (reads && targets && out))) return -1;
    for (size_t i = 0; i < n; i++) out[i] = MAP_LOCAL_NONE;
    if (c.open(model, p, [](Model *m) {
            return m->arch != 1 ? set_err("map_local_batch: model '%s' is a transducer model; reads are mapped into a longer sequence with flip-flop (CRF) models only", m->name.c_str()) : 0;
        })) return -1;
    return seq_win_batch<ShMapCrfLocalWin>(c, reads, targets, n, 0, viterbi != 0, want_path != 0, out,
        [&](const int *seq, size_t L) { return map_local_target_ok(c.fn, seq, L); },
        [&](const RunOut &ro) { ShMapCrfLocalArgs a{}; a.trans = ro.E; return a; });
}
