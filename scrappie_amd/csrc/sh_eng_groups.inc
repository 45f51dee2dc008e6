/* sh_eng_groups.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * run_device / collect / stitching, a call cut into launch groups, device-resident entry points. */

/* ------------------------------------------------------------------ */
/* public batched surface                                               */
/* ------------------------------------------------------------------ */
static long run_device(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets, const uint32_t *lengths, size_t n,
                       const scrappie_hip_params *p, const DwellJob *dw, const PostJob *pj = nullptr) {
    Model *m = get_model(e, model);
    if (!m) return -1;
    scrappie_hip_params dp = scrappie_hip_default_params();
    if (!p) p = &dp;
    if (n > e->max_launch_reads) { set_err("run_device: %zu reads exceed max_launch_reads %zu", n, e->max_launch_reads); return -1; }
    if (e->dbg_fail_run > 0 && --e->dbg_fail_run == 0) { set_err("run_device: injected failure (debug option fail_run)"); return -1; }
    const HostStamp stamp;
    if (run_pipeline(e, m, d_signal, offsets, lengths, n, p, STOP_NONE, 5, nullptr, dw, pj)) return -1;
    stamp("run_device", " on the host");
    return (long)e->current().lg.ncb;
}
extern "C" long scrappie_hip_run_device(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets,
                                        const uint32_t *lengths, size_t n, const scrappie_hip_params *p) {
    return run_device(e, model, d_signal, offsets, lengths, n, p, nullptr);
}

/* D2 + D3 of one read on the host (sh_host.c): what k_stitch does on the device.  `path` (T + 1 entries) is consumed. */
static void host_stitch_read(const Model *m, bool hp_on, const float *side, int *path, int T, bool want_pos, scrappie_hip_call &c,
                             const int *dwell = nullptr, float prior_num = 0.0f) {
    int *pos = (int *)calloc((size_t)T + 1, sizeof(int));
    if (!pos) { c.basecall = nullptr; c.basecall_length = 0; c.pos = nullptr; return; }
    char *bases;
    if (dwell) {
        bases = sh_dwell_stitch(path, dwell, T, 1, m->NS, prior_num, pos);          /* scrappie_events.c:300-321: one event per entry but the last */
    } else if (m->arch != 1) {
        if (hp_on) sh_homopolymer_side(side, path, T, m->NS);                       /* scrappie_raw.c:293 */
        bases = overlapper(path, (size_t)T + 1, m->NS - 1, pos);                    /* scrappie_raw.c:303 */
    } else {
        bases = crfpath_to_basecall(path, (size_t)T, pos);                          /* scrappie_raw.c:306 */
    }
    c.basecall = bases;
    c.basecall_length = bases ? strlen(bases) : 0;
    if (want_pos && bases) c.pos = pos; else { free(pos); c.pos = nullptr; }
}

static void stitch_range(const scrappie_hip_engine *e, const Slot &sl, const Model *m, const scrappie_hip_params *p, scrappie_hip_call *out,
                         size_t lo, size_t hi) {
    const LaunchGroup &lg = sl.lg;
    const float *scores = sl.h_score.as<float>();
    const unsigned *bad = sl.h_bad.as<unsigned>();
    for (size_t i = lo; i < hi; i++) {
        const int o = lg.order[i];
        if (o < 0) continue;
        scrappie_hip_call &c = out[o];
        c.score = NAN; c.nblock = 0; c.basecall = nullptr; c.basecall_length = 0; c.pos = nullptr;
        const int T = lg.rT[i];
        if (T <= 0) continue;
        if (bad[i]) continue;              /* input outside the split products' operand range: no call (reported by stitch_group) */
        c.score = scores[i];
        c.nblock = (size_t)T;
        if (lg.dev_stitch) {
            /* bases (and pos) were made by k_stitch: copy them out of the pinned buffers.  Reads whose homopolymer
             * mean sat on a rounding boundary (redo) are left to stitch_group. */
            if (sl.h_redo.as<unsigned>()[i] || e->dbg_redo_all) continue;
            const int len = sl.h_blen.as<int>()[i];
            if (len < 0) continue;                                   /* every entry a stay: no call (overlapper returns NULL) */
            char *bases = (char *)malloc((size_t)len + 1);
            if (!bases) continue;
            memcpy(bases, sl.h_bases.as<char>() + lg.bases_off[i], (size_t)len);
            bases[len] = 0;
            c.basecall = bases;
            c.basecall_length = (size_t)len;
            if (p->want_pos) {
                int *pos = (int *)malloc(((size_t)T + 1) * sizeof(int));
                if (pos) {
                    if (lg.dev_pos) { const int *src = sl.h_pos.as<int>() + lg.seq_off[i]; for (int t = 0; t <= T; t++) pos[t] = src[(size_t)t * SH_SEQ_STRIDE]; }
                    else memset(pos, 0, ((size_t)T + 1) * sizeof(int));             /* CRF: crfpath_to_basecall leaves pos untouched (Q11) */
                }
                c.pos = pos;
            }
            continue;
        }
        int *path = (int *)malloc(((size_t)T + 1) * sizeof(int));
        if (!path) continue;
        { const int *src = sl.h_seq.as<int>() + lg.seq_off[i]; for (int t = 0; t <= T; t++) path[t] = src[(size_t)t * SH_SEQ_STRIDE]; }
        host_stitch_read(m, lg.hp_on, lg.hp_on ? sl.h_hp.as<float>() + lg.hp_off[i] * 5 : nullptr, path, T, p->want_pos != 0, c,
                         lg.dw.on ? lg.dw.host[(size_t)o] : nullptr, lg.dw.on ? lg.dw.num[(size_t)o] : 0.0f);
        free(path);
    }
}

static int stitch_group(scrappie_hip_engine *e, Slot &sl, Model *m, const scrappie_hip_params *p, scrappie_hip_call *out, size_t n);
static void crf_post_deliver(scrappie_hip_engine *e, Slot &sl, const scrappie_hip_call *out);      /* sh_eng_crfpost.inc */

/* Host threads for stitching a launch group: the CPUs this process may actually use -- its affinity mask and its
 * cgroup CPU quota (a GPU box may report 256 CPUs and grant 16), shared with the other ranks of a torchrun job
 * (LOCAL_WORLD_SIZE) -- at most 32, SCRAPPIE_HIP_HOST_THREADS overrides.  Decided once. */
/* the CPUs this process may use: affinity mask, capped by the cgroup quota, divided among the ranks of a node */
static unsigned host_cpus() {
    static const unsigned n = [] {
        double cpus = (double)std::max(1u, std::thread::hardware_concurrency());
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) cpus = std::min(cpus, (double)CPU_COUNT(&set));
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[32]; double period = 0;
            if (fscanf(f, "%31s %lf", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) cpus = std::min(cpus, atof(q) / period);
            fclose(f);
        }
        if (const char *lw = getenv("LOCAL_WORLD_SIZE")) { const int w = atoi(lw); if (w > 1) cpus /= w; }
        return (unsigned)std::max(1.0, std::min(cpus, 4096.0));
    }();
    return n;
}
/* host threads of ONE engine (stitching, gathers): the above, at most 32 */
static unsigned host_threads() {
    static const unsigned n = [] {
        if (const char *ev = getenv("SCRAPPIE_HIP_HOST_THREADS")) { const int v = atoi(ev); if (v > 0) return (unsigned)std::min(v, 256); }
        return std::min(host_cpus(), 32u);
    }();
    return n;
}

extern "C" unsigned scrappie_hip_host_thread_budget(void) { return host_threads(); }
extern "C" unsigned scrappie_hip_host_cpu_budget(void) { return host_cpus(); }

extern "C" int scrappie_hip_collect(scrappie_hip_engine *e, const scrappie_hip_params *p, scrappie_hip_call *out, size_t n) {
    if (!e || !out) return set_err("collect: null argument");
    scrappie_hip_params dp = scrappie_hip_default_params();
    if (!p) p = &dp;
    if (!e->any_pending()) return set_err("collect: no launch group in flight");
    Slot &sl = e->slots[e->oldest].pending ? e->slots[e->oldest] : e->other(e->slots[e->oldest]);
    LaunchGroup &lg = sl.lg;
    if (!lg.valid || lg.n != n) return set_err("collect: oldest launch group has %zu reads, asked for %zu", lg.n, n);
    (void)hipSetDevice(e->device);
    const auto hs0 = std::chrono::steady_clock::now();
    if (e->ev_ok) HIPCHK(sh_event_wait(sl.done));
    else HIPCHK(sh_stream_wait(e->stream));
    const auto hs1 = std::chrono::steady_clock::now();
    struct StampOut { std::chrono::steady_clock::time_point a, b; bool on; ~StampOut() { if (on) fprintf(stderr, "host stamp: collect waited %.2f ms, then %.2f ms of host work\n", std::chrono::duration<double, std::milli>(b - a).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b).count()); } } stamp_out{hs0, hs1, tun().host_stamp};
    sl.pending = false;
    e->oldest = e->index(e->other(sl));
    if (!sl.spans.empty() && resolve_spans(e, sl)) return -1;
    Model *m = get_model(e, lg.model);
    if (!m) return -1;
    static std::atomic<bool> fake_once{false};
    const bool faked = tun().fake_timeout && e->handover && lg.ncb > 0 && !fake_once.exchange(true);
    if (lg.ncb > 0 && sl.h_err.p && (*sl.h_err.as<unsigned>() != 0 || faked)) {
        /* a state hand-over between workgroups timed out (sh_wait_flag): the results of this group are
         * invalid.  Run it again scheduled on whole tiles (no inter-workgroup waits at all), behind whatever
         * else is in flight, and stitch that. */
        if (!e->handover) return set_err("launch group failed on the device (error word set without hand-overs)");
        const std::vector<uint64_t> off = lg.in_off;
        const std::vector<uint32_t> len = lg.in_len;
        const scrappie_hip_params pp = lg.params;
        const float *dsig = lg.d_signal;
        const int other_oldest = e->oldest;
        e->handover = false;
        const DwellJob dw = lg.dw;                       /* (a copy: the re-run may take this very slot) */
        const PostJob pj = lg.post;
        const int rc = run_pipeline(e, m, dsig, off.data(), len.data(), n, &pp, STOP_NONE, 5, nullptr, &dw, &pj);
        e->handover = true;
        if (rc) return -1;
        Slot &rs = e->current();
        if (e->ev_ok) HIPCHK(sh_event_wait(rs.done)); else HIPCHK(sh_stream_wait(e->stream));
        rs.pending = false;
        e->oldest = other_oldest;
        if (!rs.spans.empty() && resolve_spans(e, rs)) return -1;
        if (*rs.h_err.as<unsigned>() != 0) return set_err("launch group failed on the device even on whole tiles");
        fprintf(stderr, "scrappie_hip: a state hand-over between workgroups timed out; launch group of %zu reads re-run on whole tiles\n", n);
        return stitch_group(e, rs, m, p, out, n);
    }
    return stitch_group(e, sl, m, p, out, n);
}

static int stitch_group(scrappie_hip_engine *e, Slot &sl, Model *m, const scrappie_hip_params *p, scrappie_hip_call *out, size_t n) {
    LaunchGroup &lg = sl.lg;
    for (size_t i = 0; i < n; i++) { out[i].score = NAN; out[i].nblock = 0; out[i].basecall = nullptr; out[i].basecall_length = 0; out[i].pos = nullptr; }
    if (lg.ncb == 0) return 0;
    {   /* reads whose input left the operand range of the split products (k_conv_act / k_feat_in): no call, said aloud */
        const unsigned *bad = sl.h_bad.as<unsigned>();
        size_t nbad = 0; long first = -1;
        for (size_t i = 0; i < lg.npad; i++) if (bad[i] && lg.order[i] >= 0) { if (!nbad || lg.order[i] < first) first = lg.order[i]; nbad++; }
        if (nbad) {
            set_err("%zu read(s) of this launch group (first: read %ld of it) hold values outside the supported range (|activation| >= %g "
                    "after the first layer, or non-finite): is the signal trimmed and med/MAD-normalised?  They get no call", nbad, first, (double)SH_ACT_LIMIT);
            fprintf(stderr, "scrappie_hip: %s\n", g_err);
        }
    }
    if (lg.dev_stitch && p->want_pos && !lg.dev_pos && m->arch != 1) {
        /* pos[] was not asked for when the group was enqueued: fetch the paths (and side rows) after all and stitch on the host */
        if (sl.h_seq.ensure((size_t)std::max<long long>(lg.nseq, 1) * 4) || (lg.hp_on && sl.h_hp.ensure((size_t)std::max<long long>(lg.nhp, 1) * 5 * 4))) return -1;
        HIPCHK(hipMemcpy(sl.h_seq.p, sl.d_seq.p, (size_t)lg.nseq * 4, hipMemcpyDeviceToHost));
        if (lg.hp_on) HIPCHK(hipMemcpy(sl.h_hp.p, sl.d_hp.p, (size_t)lg.nhp * 5 * 4, hipMemcpyDeviceToHost));
        lg.dev_stitch = false;
    }
    unsigned nthr = host_threads();
    if (e->host_thread_budget) nthr = std::min(nthr, e->host_thread_budget);
    if (lg.dev_stitch) nthr = std::min(nthr, 4u);             /* copying strings out of pinned memory: a few ms on one thread */
    if (lg.npad < 256) nthr = 1;
    if (nthr == 1) stitch_range(e, sl, m, p, out, 0, lg.npad);
    else {
        std::vector<std::thread> th;
        const size_t per = (lg.npad + nthr - 1) / nthr;
        for (unsigned t = 0; t < nthr; t++) {
            const size_t lo = t * per, hi = std::min(lg.npad, lo + per);
            if (lo >= hi) break;
            th.emplace_back(stitch_range, e, std::cref(sl), m, p, out, lo, hi);
        }
        for (auto &x : th) x.join();
    }
    if (lg.dev_stitch) {
        /* reads k_stitch would not decide (a homopolymer run's posterior-mean count within rounding noise of a boundary):
         * their path and side rows are still on the device; the host code decides */
        const unsigned *redo = sl.h_redo.as<unsigned>();
        const unsigned *bad = sl.h_bad.as<unsigned>();
        size_t nredo = 0;
        for (size_t i = 0; i < lg.npad; i++) {
            const int o = lg.order[i], T = lg.rT[i];
            if (o < 0 || T <= 0 || bad[i] || !(redo[i] || e->dbg_redo_all)) continue;
            std::vector<int> path((size_t)T + 1);
            std::vector<float> side(lg.hp_on ? (size_t)T * 5 : 0);
            HIPCHK(hipMemcpy2D(path.data(), 4, sl.d_seq.as<int>() + lg.seq_off[i], (size_t)SH_SEQ_STRIDE * 4, 4, (size_t)T + 1, hipMemcpyDeviceToHost));
            if (lg.hp_on) HIPCHK(hipMemcpy(side.data(), sl.d_hp.as<float>() + lg.hp_off[i] * 5, (size_t)T * 5 * 4, hipMemcpyDeviceToHost));
            host_stitch_read(m, lg.hp_on, side.data(), path.data(), T, p->want_pos != 0, out[o],
                             lg.dw.on ? lg.dw.host[(size_t)o] : nullptr, lg.dw.on ? lg.dw.num[(size_t)o] : 0.0f);
            nredo++;
        }
        e->n_redo += nredo;
    }
    if (lg.post.on) crf_post_deliver(e, sl, out);
    return 0;
}

/* Launch groups of one call, two in flight: group g+1 is planned, staged and enqueued before the host
 * waits for group g and stitches it.  The call's reads are SORTED BY LENGTH (longest first, stable) before they are
 * cut into groups: a group lasts at least as long as its longest read's serial chain, so a long read should share
 * its group with other long reads, not hold a group of short ones hostage (DESIGN.md section 7, mixed lengths).
 * stage(k, idx, cnt) makes the signals of reads idx[0..cnt) of the call available on the device and returns the
 * pointer/offset/length arrays to run them with. */
struct GroupArgs { const float *d; const uint64_t *off; const uint32_t *len; const DwellJob *dw = nullptr; const PostJob *pj = nullptr; };      /* (dw: events with the dwell correction, the group's dwells; pj: a flip-flop group's base probabilities) */

/* the last launch group of a streaming call (scrappie_hip_basecall_device_stream), still in flight when the call returned: collected by
 * the next call on the engine -- behind that call's first launch -- or by scrappie_hip_stream_flush */
static int collect_carry(scrappie_hip_engine *e) {
    auto &c = e->carry;
    if (!c.live) return 0;
    c.live = false;
    std::vector<scrappie_hip_call> tmp(c.perm.size());
    if (scrappie_hip_collect(e, &c.p, tmp.data(), tmp.size())) { scrappie_hip_free_calls(tmp.data(), tmp.size()); return -1; }
    for (size_t i = 0; i < tmp.size(); i++) c.out[c.perm[i]] = tmp[i];
    return 0;
}

/* `where` (may be null): read i of the call delivers into out[where[i]] instead of out[i] (a call that runs a subset of its caller's
 * reads: device_deferred) */
template <class Stage>
static int run_groups(scrappie_hip_engine *e, int model, const Model *m, const uint32_t *all_len, size_t n,
                      const scrappie_hip_params *p, scrappie_hip_call *out, Stage stage, bool stream = false, const size_t *where = nullptr) {
    scrappie_hip_params dp = scrappie_hip_default_params();
    if (!p) p = &dp;
    if (!stream && e->carry.live && collect_carry(e)) return -1;      /* an ordinary call behind a streaming one: that one's last group first */
    const int inflight = (e->slots[0].pending ? 1 : 0) + (e->slots[1].pending ? 1 : 0);
    if (inflight > (e->carry.live ? 1 : 0)) return set_err("launch groups are already in flight on this engine: collect them first");
    if (n == 0) return 0;
    const int unit = m->arch == 3 ? 1 : std::max(m->stride, 1);    /* events models: lengths already count blocks */
    std::vector<uint32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    /* (the decoder-input and trunk-input hooks address their data by a read's position in its launch group: input order) */
    if (!tun().input_order && !e->alt_prob && !e->alt_trunk) std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return all_len[a] > all_len[b]; });
    std::vector<uint32_t> sorted_len(n);
    for (size_t i = 0; i < n; i++) sorted_len[i] = all_len[perm[i]];
    std::vector<size_t> starts(n);
    const long ng = scrappie_hip_plan_groups(sorted_len.data(), n, unit, e->max_launch_reads, launch_block_cap(e, m), starts.data(), n);
    if (ng < 0) return set_err("a read is too long for one launch group on this device");
    starts.resize((size_t)ng); starts.push_back(n);
    auto at = [&](size_t i) -> scrappie_hip_call & { return out[where ? where[i] : i]; };
    auto blank = [&]() { for (size_t i = 0; i < n; i++) { scrappie_hip_call &c = at(i); c.score = NAN; c.nblock = 0; c.basecall = nullptr; c.basecall_length = 0; c.pos = nullptr; } };
    blank();
    auto fail = [&]() {   /* leave the engine drained; a failed call returns nothing: release the calls already stitched */
        e->drain();
        e->carry.live = false;                 /* (a carried group's reads keep their blank entries: the stream has failed) */
        const std::string keep = g_err;
        for (size_t i = 0; i < n; i++) scrappie_hip_free_calls(&at(i), 1);
        blank();
        set_err("%s", keep.c_str());
        return -1;
    };
    std::vector<scrappie_hip_call> tmp;
    auto collect = [&](size_t g) {      /* the group's calls come back in the group's order: hand them to their reads */
        const size_t lo = starts[g], cnt = starts[g + 1] - lo;
        tmp.assign(cnt, scrappie_hip_call{});      /* (never the previous group's pointers: out[] owns those; a failed collect frees what tmp holds) */
        if (scrappie_hip_collect(e, p, tmp.data(), cnt)) { scrappie_hip_free_calls(tmp.data(), cnt); return -1; }
        for (size_t i = 0; i < cnt; i++) at(perm[lo + i]) = tmp[i];
        return 0;
    };
    size_t prev = 0; bool have_prev = false;
    /* (the staging slot of this call's group g: the carried group, if any, sits in the slot the previous call used last) */
    const int slot0 = e->carry.live ? (e->carry.slot ^ 1) : 0;
    for (long g = 0; g < ng; g++) {
        const size_t lo = starts[g], cnt = starts[g + 1] - lo;
        GroupArgs a;
        int rc = stage((int)((g + slot0) & 1), perm.data() + lo, cnt, a);
        if (!rc && run_device(e, model, a.d, a.off, a.len, cnt, p, a.dw, a.pj) < 0) rc = -1;
        if (e->carry.live) { if (collect_carry(e)) rc = -1; }          /* the previous call's last group, behind this call's first launch */
        else if (have_prev && collect(prev)) rc = -1;
        have_prev = false;
        if (rc) return fail();
        prev = (size_t)g; have_prev = true;
    }
    if (have_prev && stream) {                  /* leave the last group running: the pipeline does not drain between calls */
        const size_t lo = starts[prev], cnt = starts[prev + 1] - lo;
        e->carry.perm.assign(perm.begin() + (long)lo, perm.begin() + (long)(lo + cnt));
        if (where) for (auto &x : e->carry.perm) x = (uint32_t)where[x];      /* (the caller's vector is gone by the time the group is delivered) */
        e->carry.out = out; e->carry.p = *p; e->carry.slot = (int)((prev + slot0) & 1); e->carry.live = true;
        return 0;
    }
    if (have_prev && collect(prev)) return fail();
    return 0;
}

static int basecall_device(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets, const uint32_t *lengths, size_t n,
                           const scrappie_hip_params *p, scrappie_hip_call *out, bool stream) {
    if (!e || !out) return set_err("basecall_device%s: null argument", stream ? "_stream" : "");
    Model *m = get_model(e, model);
    if (!m) return -1;
    std::vector<uint64_t> off[2];
    std::vector<uint32_t> len[2];
    return run_groups(e, model, m, lengths, n, p, out, [&](int k, const uint32_t *idx, size_t cnt, GroupArgs &a) {
        off[k].resize(cnt); len[k].resize(cnt);
        for (size_t i = 0; i < cnt; i++) { off[k][i] = offsets[idx[i]]; len[k][i] = lengths[idx[i]]; }
        a.d = d_signal; a.off = off[k].data(); a.len = len[k].data();
        return 0;
    }, stream);
}
extern "C" int scrappie_hip_basecall_device(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets,
                                            const uint32_t *lengths, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out) {
    return basecall_device(e, model, d_signal, offsets, lengths, n, p, out, false);
}

/* scrappie_hip_basecall_device that returns while its LAST launch group is still running.  That group's calls are delivered -- into the
 * same out[] -- by the next scrappie_hip_basecall_device_stream call on the engine, behind that call's first launch (so the pipeline of
 * two groups in flight never drains between batches), or by scrappie_hip_stream_flush; until then their out[] entries are blank.  out[]
 * and d_signal of a call must stay valid until its last group has been delivered.  Any other batched call on the engine delivers the
 * carried group first.  A failure loses the carried group's calls too (their entries stay blank): the stream has failed. */
extern "C" int scrappie_hip_basecall_device_stream(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets,
                                                   const uint32_t *lengths, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out) {
    return basecall_device(e, model, d_signal, offsets, lengths, n, p, out, true);
}
extern "C" int scrappie_hip_stream_flush(scrappie_hip_engine *e) {
    if (!e) return set_err("stream_flush: null engine");
    if (!e->carry.live) return 0;
    (void)hipSetDevice(e->device);
    if (collect_carry(e)) {
        const std::string keep = g_err;
        e->drain();
        return set_err("%s", keep.c_str());
    }
    return 0;
}

/* Arenas before the first real call: a launch group of n reads of `samples` samples each (all-zero signals) is run and thrown away, so
 * that every device and pinned buffer a group of that shape needs exists (hipMalloc / hipFree of gigabytes synchronise the device: a
 * call that grows its arenas stalls whatever else is running) and the kernels' code objects are resident.  `scrappie raw` calls it
 * while its loader reads the first full batch. */
extern "C" int scrappie_hip_warm_up(scrappie_hip_engine *e, int model, size_t n, size_t samples) {
    if (!e) return set_err("warm_up: null engine");
    Model *m = get_model(e, model);
    if (!m) return -1;
    if (n == 0 || samples == 0) return 0;
    (void)hipSetDevice(e->device);
    const size_t per = m->arch == 3 ? (size_t)m->nfeat : 1;
    float *d = nullptr;
    HIPCHK(hipMalloc(&d, n * samples * per * 4));
    int rc = hipMemset(d, 0, n * samples * per * 4) == hipSuccess ? 0 : set_err("warm_up: hipMemset failed");
    if (!rc) {
        std::vector<uint64_t> off(n);
        std::vector<uint32_t> len(n, (uint32_t)samples);
        for (size_t i = 0; i < n; i++) off[i] = (uint64_t)i * samples * per;
        std::vector<scrappie_hip_call> calls(n);
        rc = scrappie_hip_basecall_device(e, model, d, off.data(), len.data(), n, nullptr, calls.data());
        if (!rc) scrappie_hip_free_calls(calls.data(), n);
    }
    (void)hipFree(d);
    return rc;
}
