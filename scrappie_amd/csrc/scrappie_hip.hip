/* scrappie_hip.hip -- engine + C ABI of libscrappie_hip.so (gfx950 only).
 *
 * One engine = one GPU, three HIP streams (kernels; results -> host; host signals -> device),
 * grow-only device arena sized for HBM (a launch group is bounded by device memory: about 100 KB per
 * tile and block for the transducer models).  Reads handed to the engine are coalesced into LAUNCH
 * GROUPS: sorted by block count, cut into tiles of 16, and pushed through
 *
 *   rgrgr / rnnrf:   k_conv_act -> 5 x k_gru_proj (projection team + recurrence team, gate inputs in LDS)
 *                    -> k_ff_viterbi (S1 inside the decoder; 4^5 + 1 states over 96 units)
 *                       | k_ff_lds / k_ff_exp -> k_viterbi                       (other shapes, posterior wanted)
 *                    -> k_walk_stitch_out (walk back + homopolymer pass + stitching + results to pinned host memory, copy stream;
 *                       SH_SPLIT_TAIL, host stitching, no copy stream: k_backtrace -> k_stitch -> k_results_out)   (rnnrf: k_affine -> k_crf -> k_stitch -> k_results_out)
 *   input != state width, S not in {32, 64, 96}, SH_GRU_SEPARATE:
 *                    ... 5 x (k_affine[_lds] -> k_gru_split | k_gru) ...
 *   raw_r94:         k_conv_act -> 2 x {k_gru_proj fwd, bwd -> k_affine2_tanh} -> S1 -> decode
 *   events:          k_feat_in -> 2 x {k_lstm_proj fwd, bwd (projection + peephole LSTM in one kernel) -> k_affine2_tanh} -> S1 -> decode
 *                    (SH_GRU_SEPARATE: k_affine + k_lstm_lanes)
 *   a GRU layer with a weight outside the split products' operand range (|w| >= 255): k_affine<.., F32> -> k_gru_lanes (exact fp32)
 *
 * The contractions of the projection, the recurrence and S1 run as split products on the f16 matrix pipe
 * (sh_kernels.h, split_pair / split_dot): fp32 in, fp32 out, fp32 accuracy.  The recurrent kernels and the two-team
 * decoder walk a lane schedule, the other decoder kernels work on pieces of tiles (sh_sched.h).  Two launch groups can be in flight: the host stitches
 * group k (homopolymer correction, k-mer overlap: sh_host.c, C) while group k+1 runs.  Only decoded paths
 * (and the 5-row homopolymer side buffer) cross PCIe.
 *
 * The translation unit in parts (round 5; the kernels are templates in headers and are instantiated where they are launched, so
 * the engine stays ONE translation unit -- the parts are files of their own for reading, included below in this order):
 *   this file            launch_k / pick_int / pick_bool / StampBuf (how every kernel is launched), switches, the engine's state (struct Slot: what
 *                        exists once per launch group in flight), create / destroy
 *   sh_eng_weights.inc   weights as the device wants them; the Model
 *   sh_eng_load.inc      .scrm container -> Model, settings, the ABI's planning functions
 *   sh_eng_launch.inc    launch-group construction; kernel dispatch helpers: a layer's sizes and switches -> the instantiation that runs
 *   sh_eng_pipeline.inc  run_pipeline: one launch group through its kernels, a function per stage
 *   sh_eng_groups.inc    run_device / collect / stitching, a call cut into launch groups
 *   sh_eng_batch.inc     helper engine for chain-bound reads, host-signal entry points, several GPUs
 *   sh_eng_debug.inc     measurement / test hooks
 *   sh_eng_surface.inc   the reference's per-read functions: one batch function per family, run by the queue or with a batch of one
 *   sh_eng_cut.inc       what the engines below share: a call cut into launches that fit the device (LaunchCut), per-read DP
 *                        records through a kernel with two homes (dp_order / dp_launch / dp_collect)
 *   sh_eng_post.inc      what the engines on a launch group's posterior or transitions share: the batch call and its memory model
 *                        (PostCall), the launch group's stage (post_group), one plan and runner for two homes (DpPlan / dp_run), sets of
 *                        short sequences in packs (PackSet / PackLaunch), a host matrix's upload, the two-span timer
 *   sh_eng_win.inc       what the engines that map INTO a longer reference share: a reference cut into windows (WinCut / win_cut), both passes over
 *                        the windows of a launch for a family's WinTraits (win_launch / win_run), the windows' forward sum (win_lse), what a read
 *                        adds to a launch (win_read_bytes); for the two on a launch group's posterior or transitions the sequences' upload, the
 *                        launch group's stage and the batch call (seq_win_run / seq_win_batch)
 *   sh_eng_map_crf.inc   mapping of flip-flop (CRF) reads to base sequences (per-read; the launch group of the batched call)
 *   sh_eng_map.inc       block-based mapping of posteriors to sequences (per-read and batched)
 *   sh_eng_cands.inc     what the two engines that score one read against many candidate sequences packed into workgroups share: the set of a cand
 *                        array (cand_set_build), its packs and the left-over candidates of a launch (cand_run), the launch group with its second
 *                        pass and the batch call (cand_group / cand_batch), the per-read symbol's tail (cand_one), the result type's release, form counts
 *   sh_eng_map_pack.inc  the CandTraits of the transducer models (k_map_pack), their checks and entry points
 *   sh_eng_map_crf_pack.inc  the CandTraits of the flip-flop (CRF) models (k_map_crf_pack), their checks and entry points
 *   sh_eng_edits.inc     what the two engines that score every single-base edit of a sequence share: forward rows, backward rows and one combining
 *                        pass per launch for a family's EditsTraits (edits_launch), the cut by a byte budget (edits_run), the per-read symbol's
 *                        tail (edits_one), the batch call (edits_batch), the result type's release, form counts and timing
 *   sh_eng_crf_edits.inc the EditsTraits of the flip-flop (CRF) models (k_crf_edits_rows, k_crf_edits), their checks and entry points
 *   sh_eng_map_edits.inc the EditsTraits of the transducer models (k_map_edits_rows, k_map_edits), their checks and entry points
 *   sh_eng_crf_find.inc  short sequences searched inside flip-flop (CRF) reads, packed into workgroups (per-read and batched)
 *   sh_eng_map_crf_local.inc  flip-flop (CRF) reads mapped into a longer sequence, one workgroup per window (per-read and batched)
 *   sh_eng_map_local.inc      transducer reads mapped into a longer sequence, one workgroup per window, the posterior column staged in LDS (per-read and batched)
 *   sh_eng_squig.inc     mapping of raw signals to predicted squiggles (per-read and batched)
 *   sh_eng_squig_pack.inc  one signal against many candidate squiggles, packed into workgroups
 *   sh_eng_squig_local.inc  raw signals mapped into a longer reference squiggle, one workgroup per window (per-read and batched)
 *   sh_eng_sqnet.inc     prediction of squiggles from base sequences (per-read and batched)
 *   sh_eng_events.inc    event detection (per-read and batched; kernels in sh_events.h)
 *   sh_eng_crfpost.inc   base probabilities of the flip-flop models (k_crf_post, sh_crf_post.h): inside a launch group and on host matrices
 * Separate translation units: sh_p0.hip (signal preparation, k_p0), sh_host.c / sh_fast5.c / sh_h5mini.c (host C);
 * sh_coalesce.h (the per-read functions' queue) and sh_dev.h (DBuf / HBuf: buffers that own their memory) are plain C++ headers.
 */
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <set>

#include "scrappie_hip.h"
#include "sh_internal.h"
#include "sh_kernels.h"
#include "sh_sched.h"
#include "sh_dev.h"
#include "sh_coalesce.h"
#include "sh_map.h"
#include "sh_map_pack.h"
#include "sh_squig.h"
#include "sh_squig_band.h"
#include "sh_squig_pack.h"
#include "sh_squig_local.h"
#include "sh_sqnet.h"
#include "sh_events.h"

/* function attributes (dynamic LDS limit) are per device: remember for which devices a kernel has had its attribute set
 * (engines on several GPUs may share one process).  A real once per device: the thread that finds the attribute unset holds
 * the lock until the call that sets it has returned (`if (auto turn = once.first()) HIPCHK(...);` in launch_k below -- the
 * turn lives to the end of the if statement), so a second engine on the same device -- the helper engine runs launch groups
 * on a host thread of its own -- cannot launch the kernel with more than 64 KB of dynamic LDS before the limit is raised. */
struct DevOnce {
    std::atomic<unsigned long long> done{0};
    std::mutex mu;
    struct Turn {
        DevOnce *o; unsigned long long bit;
        Turn(DevOnce *o_, unsigned long long b_) : o(o_), bit(b_) {}
        Turn(Turn &&t) : o(t.o), bit(t.bit) { t.o = nullptr; }
        Turn(const Turn &) = delete;
        explicit operator bool() const { return o != nullptr; }
        ~Turn() { if (o) { o->done.fetch_or(bit, std::memory_order_release); o->mu.unlock(); } }
    };
    Turn first(bool wanted = true) {
        if (!wanted) return Turn(nullptr, 0);
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (done.load(std::memory_order_acquire) & bit) return Turn(nullptr, 0);
        mu.lock();
        if (done.load(std::memory_order_acquire) & bit) { mu.unlock(); return Turn(nullptr, 0); }
        return Turn(this, bit);
    }
};

/* The one place a kernel is launched with dynamic LDS.  K names the instantiation (`launch_k<k_gru_proj<6, 2, false>>(...)`), and every instantiation
 * has a DevOnce of its own: attr_once<K>, which hangs on K alone, not on the types a launch passes its arguments as.  One rule for all kernels: a
 * launch that asks for more than 48 KB raises K's limit to the device's 160 KB first, once per device and under the once's turn (above: a second engine's thread cannot launch K before the limit is up).  48 KB is the most conservative threshold
 * the launchers ever used; those that used to set the limit at a smaller size as well no longer do, which changes nothing: the default limit covers
 * such a launch.  Arguments are passed as given and converted where the kernel is called: a kernel's default arguments do not exist through K, so a
 * launch spells them out.  Returns 0, or -1 through HIPCHK; the launch's own error is left to the caller's hipGetLastError, as with a plain launch. */
template <auto K>
static DevOnce &attr_once() { static DevOnce once; return once; }
template <auto K, class... A>
static int launch_k(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &...a) {
    if (auto turn_ = attr_once<K>().first(lds > 48 * 1024))
        HIPCHK(hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(K, grid, block, lds, s, a...);
    return 0;
}

/* Run-time values as template arguments.  pick_int<2, 4, 6>(v, rc, f): rc = f(int_c<V>()) for the V of the list that equals v; false (f not called,
 * rc untouched) where none does, so that the caller words the refusal.  pick_bool(f, b...): f with std::true_type() or std::false_type() for every b,
 * in their order; returns what f returns.  f is a generic lambda that takes the constants by value (`[&](auto nu) { return launch_k<k_gru<nu()>>(...); }`;
 * a lambda nested in f names the value through a constexpr of f's, not through f's parameter).  Every V of the list, and both values of every b,
 * instantiate f's body: a kernel family that uses part of a cross product leaves the rest out with `if constexpr`. */
template <int V> using int_c = std::integral_constant<int, V>;
template <int... Vs, class F>
static bool pick_int(int v, int &rc, F &&f) {
    return ((v == Vs && ((rc = f(int_c<Vs>())), true)) || ...);
}
template <class F>
static int pick_bool(F &&f) { return f(); }
template <class F, class... B>
static int pick_bool(F &&f, bool b, B... rest) {
    return b ? pick_bool([&](auto... c) { return f(std::true_type(), c...); }, rest...)
             : pick_bool([&](auto... c) { return f(std::false_type(), c...); }, rest...);
}

/* Cycle stamps of an instrumented kernel form (development switches; tools/ab_stamp.sh and tools/profile_gru32.sh read the lines): a device buffer
 * allocated on first use, and dump_on(k, ...): on the k-th call (k = 0: on every call) wait for the stream, bring `words` words back and hand them
 * to print(const unsigned long long *).  One per stamped form, with static storage: single-threaded use, never freed. */
struct StampBuf {
    unsigned long long *d = nullptr;
    int calls = 0;
    unsigned long long *dev(size_t words) {
        if (!d) (void)hipMalloc(&d, words * 8);
        return d;
    }
    template <class P>
    void dump_on(int k, hipStream_t s, size_t words, P &&print) {
        if (k && ++calls != k) return;
        (void)sh_stream_wait(s);
        std::vector<unsigned long long> h(words);
        (void)hipMemcpy(h.data(), d, words * 8, hipMemcpyDeviceToHost);
        print(h.data());
    }
};

/* Development switches (kernel-family selection, cycle stamps).  Read from the environment ONCE, when the
 * first engine is created -- never on the launch path. */
struct Tunables {
    bool affine_reg, gru_single, gru_stamp, gru_separate, gru_f32, gru_lanes_stamp, proj_stamp, ff_reg, ff_stamp, vit_stamp, ff_separate, fv_single, host_stamp, host_stitch, split_tail, helper_fence, gru_free, gru_barrier, input_order, conv_valu, conv_in_layer, gru32, gru16, gru32_stamp;
    int gru_debug;       /* -1: off */
    int conv_tchunk;     /* blocks per workgroup pass of k_conv_act (SH_CONV_TCHUNK, default 16) */
    double gru_two_ratio; /* step time of a two-tile workgroup of k_gru_proj over a one-tile one (SH_GRU_TWO_RATIO, default 1.8) */
    bool fake_timeout;   /* SH_FAKE_HANDOVER_TIMEOUT: collect() treats the first launch group as timed out (test hook) */
    Tunables() {
        auto on = [](const char *k) { return getenv(k) != nullptr; };
        /* experiment switches (kernel forms measured and not adopted, cycle stamps, scheduling experiments) exist only in the experiments
         * build (-DSH_EXPERIMENTS: libscrappie_hip_exp.so, what the tests of those forms load); the product library does not carry the kernels */
#ifdef SH_EXPERIMENTS
        auto xon = on;
#else
        auto xon = [](const char *) { return false; };
#endif
        affine_reg = xon("SH_AFFINE_REG"); gru_single = xon("SH_GRU_SINGLE"); gru_stamp = xon("SH_GRU_STAMP");
        gru_separate = on("SH_GRU_SEPARATE"); gru_f32 = on("SH_GRU_F32"); gru_lanes_stamp = xon("SH_GRU_LANES_STAMP");
        proj_stamp = xon("SH_PROJ_STAMP"); ff_reg = xon("SH_FF_REG"); ff_stamp = xon("SH_FF_STAMP"); vit_stamp = xon("SH_VIT_STAMP");
        host_stamp = xon("SH_HOST_STAMP");         /* host-side wall times of a launch group on stderr */
        gru_free = xon("SH_GRU_FREE");             /* recurrent layers on k_gru_free (no s_barrier in the step loop: LDS counters) */
        gru_barrier = xon("SH_GRU_BARRIER");       /* ... on k_gru_proj (two s_barriers per step shared by both teams) */
        helper_fence = xon("SH_HELPER_FENCE");     /* experiment: the first recurrent layer waits for the previous group's traceback walk + k_stitch */
        split_tail = on("SH_SPLIT_TAIL");         /* walk back, stitching and result transfer as three kernels (k_backtrace, k_stitch, k_results_out) where k_walk_stitch_out applies */
        host_stitch = on("SH_HOST_STITCH");       /* homopolymer correction + k-mer stitching on host threads (paths + 5 rows over PCIe) instead of k_stitch */
        gru32 = xon("SH_GRU32");                   /* recurrent layers of S = 96 on tiles of 32 reads (k_gru_proj32) */
        gru16 = xon("SH_GRU16");                   /* ... on tiles of 16 reads (k_gru_proj) */
        gru32_stamp = xon("SH_GRU32_STAMP");       /* ... with cycle stamps of one launch on stderr */
        conv_in_layer = xon("SH_CONV_IN_LAYER");   /* experiment (measured 1 ms per step SLOWER): the first recurrent layer of the rgrgr models computes the convolution itself (k_gru_conv) */
        conv_valu = on("SH_CONV_VALU");           /* the convolution as VALU multiplies and additions (k_conv_act) where k_conv_mfma applies */
        input_order = xon("SH_INPUT_ORDER");       /* experiment: a call's launch groups cut in input order instead of sorted by length */
        ff_separate = on("SH_FF_SEPARATE");      /* S1 and the decoder as two kernels even where k_ff_viterbi applies */
        fv_single = on("SH_FV_SINGLE");          /* S1 inside the decoder on eight do-everything waves (k_ff_viterbi) instead of two teams (k_ff_viterbi_teams) */
        fake_timeout = on("SH_FAKE_HANDOVER_TIMEOUT");
#ifdef SH_EXPERIMENTS
        const char *dm = getenv("SH_GRU_DEBUG");
#else
        const char *dm = nullptr;
#endif
        gru_debug = dm ? atoi(dm) : -1;
        const char *tc = getenv("SH_CONV_TCHUNK");
        conv_tchunk = tc ? std::max(1, std::min(atoi(tc), 256)) : 16;
        const char *tr = getenv("SH_GRU_TWO_RATIO");
        gru_two_ratio = tr ? atof(tr) : 1.8;
    }
};
static const Tunables &tun() { static const Tunables t; return t; }

#ifndef SH_GRU_FREE_DEFAULT
#define SH_GRU_FREE_DEFAULT 0     /* 1: recurrent layers run k_gru_free unless SH_GRU_BARRIER is set; 0: k_gru_proj unless SH_GRU_FREE is set */
#endif
#ifndef SH_AFF_NB
#define SH_AFF_NB 3      /* column blocks per wave in k_affine_lds */
#endif
#ifndef SH_AFF_NTH
#define SH_AFF_NTH 512   /* threads per workgroup in k_affine_lds */
#endif
#ifndef SH_FF_NB
#define SH_FF_NB 4     /* column blocks per wave in k_ff_exp */
#endif

/* errors (thread-local text behind scrappie_hip_last_error), HIPCHK, grow-only device / pinned buffers: sh_dev.h */
static thread_local char g_err[512] = "";
int sh_set_err_v(const char *fmt, va_list ap) {
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    return -1;
}
extern "C" const char *scrappie_hip_last_error(void) { return g_err; }
extern "C" void sh_set_error(const char *fmt, ...) {       /* (sh_host.c: the host C sets the same text) */
    va_list ap;
    va_start(ap, fmt);
    (void)sh_set_err_v(fmt, ap);
    va_end(ap);
}

#include "sh_eng_weights.inc"      /* weights as the device wants them: MFMA fragments, fp16 pieces, bias tables; the Model */
/* ------------------------------------------------------------------ */
/* engine                                                               */
/* ------------------------------------------------------------------ */
/* The dwell correction of an events launch group (sh_dwell.h): what its stage hands over beside the feature matrices (GroupArgs -> run_pipeline -> build_group).  Per read of the group, in the
 * group's own order: where its dwells are in d_dwell, the prior's numerator, and the dwells on the host -- what the host statement needs for a read the
 * device leaves to it; they outlive the group's collection (the call owns them). */
struct DwellJob {
    bool on = false;
    const int *d_dwell = nullptr;
    std::vector<uint64_t> off;
    std::vector<float> num;
    std::vector<const int *> host;
};

/* The base probabilities of a flip-flop launch group (k_crf_post, sh_eng_crfpost.inc), handed over like the dwell job: per read of the group, in the
 * group's own order, where its matrix is to be delivered (the call owns the places). */
struct PostJob {
    bool on = false;
    std::vector<scrappie_matrix *> dst;
};

struct LaunchGroup {
    PostJob post;                 /* base probabilities wanted (build_group takes its caller's) */
    std::vector<long long> post_off;      /* ... where each read's (T + 1) x 5 floats lie in the slot's buffer (tiled order; scrappie_hip_crf_post_plan) */
    long long npost = 0;          /* ... and the floats of all of them */
    DwellJob dw;                  /* events with the dwell correction on: the group's dwells (build_group takes its caller's) */
    size_t n = 0, npad = 0, ntile = 0;
    long long ncb = 0;            /* total column blocks */
    long long nseq = 0;           /* total path ints */
    long long nhp = 0;            /* total blocks of real reads (hp side rows) */
    std::vector<int> order;       /* tiled index -> original read index (or -1) */
    std::vector<int> rT, rN;
    std::vector<long long> tile_boff;     /* per tile: its first column block */
    std::vector<long long> seq_off, hp_off, bases_off;
    long long nbases_cap = 0;     /* bytes of the per-slot bases buffer (k_stitch) */
    bool dev_stitch = false;      /* bases were made on the device (k_stitch); else paths (+ side rows) come to the host */
    bool dev_pos = false;         /* ... and pos[] too */
    int model = -1;
    bool hp_on = false;
    bool valid = false;
    int gru_nwg = 0;              /* lane schedule of the recurrent kernel (sh_sched.h) */
    int gru1_nwg = 0;             /* ... with one lane per workgroup (k_gru_proj with fewer tiles than CUs) */
    bool gru_two = false;         /* more live tiles than CUs: k_gru_proj steps two tiles per workgroup */
    int gru32_nwg = 0;            /* ... over pairs of tiles, one pair at a time per workgroup (k_gru_proj32) */
    int gru32x2_nwg = 0;          /* ... two pairs at a time per workgroup (k_gru_proj32x2) */
    int vit_nwg = 0;              /* ... and of the Viterbi decoder: pieces of tiles, one per workgroup (k_viterbi, k_ff_viterbi) */
    int vit_lane_nwg = 0;         /* ... and its lane layout (k_ff_viterbi_teams): workgroups, */
    int vit_lane_nseg = 0;        /* and the segments they walk */
    int vit_launched = 0;         /* segments of the decoder launch that ran (the "decoder_pieces" debug fetch), */
    int vit_launched_wg = 0;      /* and its workgroups ("decoder_wgs") */
    /* what the group was launched with, kept so that scrappie_hip_collect can run it again on whole tiles
     * should a state hand-over between workgroups time out */
    const float *d_signal = nullptr;
    std::vector<uint64_t> in_off;
    std::vector<uint32_t> in_len;
    scrappie_hip_params params{};
};

/* scrappie_hip_basecall_batch from several host threads (sh_eng_batch.inc): the requests that are waiting for one engine run as one engine call */
struct BatchReq {
    scrappie_hip_engine *e = nullptr;
    int model = 0;
    const raw_table *reads = nullptr;
    size_t n = 0;
    scrappie_hip_params p{};
    scrappie_hip_call *out = nullptr;
    int rc = -1;
    std::string err;
    int phase = 0;                   /* sh_coalesce.h: 0 queued ... 3 done */
};
struct BatchCoalescer : ShCoalescer<BatchReq> { BatchCoalescer() { target_pct = 100; window_mul = 4; } };      /* a leader waits for every thread seen inside lately (sh_coalesce.h) */

/* the posteriors of a launch of the per-read functions in pinned memory: every caller copies its own matrix out after the engine's lock is released
 * (all at once) and counts itself off `users`; the buffer is written again only when nobody is left (sh_eng_surface.inc) */
struct PostStage { HBuf h; DBuf d; std::atomic<int> users{0}; };

/* The device side of per-read DP records run through a kernel with two homes (k_map, k_squig: score rows in LDS or in device scratch; dp_launch and
 * dp_collect, sh_eng_cut.inc): the records in device order, traceback, scratch rows, score and final state per record, and for the walk back the
 * records' path offsets and the paths.  h (pinned) brings scores | paths back; a family may stage its uploads in it first.  Grow-only. */
struct DpBufs {
    DBuf rd, tb, scr, score, final_state, path_off, paths;
    HBuf h;
    /* fs_bytes: of a record's final-state entry (an int; k_map_crf_local's end cell is an int2) */
    int ensure(size_t n, size_t rec_bytes, long long tb_words, long long scr_floats, long long path_len, size_t h_bytes = 0, size_t fs_bytes = 4) {
        return (rd.ensure(n * rec_bytes) || tb.ensure((size_t)tb_words * 4 + 16) || scr.ensure((size_t)scr_floats * 4 + 16) || score.ensure(n * 4 + 16) ||
                final_state.ensure(n * fs_bytes + 16) || path_off.ensure(n * 8) || paths.ensure((size_t)path_len * 4 + 16) ||
                h.ensure(std::max(h_bytes, n * 4 + (size_t)path_len * 4))) ? -1 : 0;
    }
};

/* What an engine keeps for one family of "every single-base edit" (sh_eng_edits.inc): a launch's records, codes, row matrices, results and base scores,
 * results | base scores on the host (grow-only); budget: row and result bytes one launch of the three kernels may hold (debug options
 * "crf_edits_budget_kb" / "map_edits_budget_kb"; 0: one launch per launch group); the last call's kernels by events, its launches and their row bytes. */
struct EditsState { DBuf rd, seq, rows, res, base; HBuf h; size_t budget = 0; double ms[3] = {0, 0, 0}; size_t launches = 0, row_bytes = 0; };

/* What an engine keeps for one family of candidates in packs (sh_eng_cands.inc): a launch's pack records, their cell words, first cells (k_map_pack's alone) and
 * scores, scores on the host (grow-only); cells: what a pack holds (debug options "map_pack_cells" / "map_crf_pack_cells"; 0: every candidate through the
 * per-candidate kernel, -1: the family's default). */
struct PackState { DBuf rd, cell, first, score; HBuf h; int cells = -1; };

/* fields of scrappie_hip_timing (and two figures of SH_HOST_STAMP) that a span between two profiling marks adds to: resolve_spans (sh_eng_load.inc) */
enum SpanField { F_CONV = 0, F_AFFINE, F_GRU, F_FF, F_DECODE, F_BACKTRACE, F_TOTAL, F_FUSED, F_STITCH,
                 F_WAIT, F_LEAD,      /* how long the main stream waited for the prologue; how long before that the convolution had ended */
                 F_COUNT };

/* Everything that exists once per launch group in flight.  The engine keeps two, so group k+1 can be enqueued while the host is still stitching
 * group k: its metadata, staged signals, convolution output, the device buffers the host reads back (a second stream copies them out while the
 * next group computes) and their pinned twins, its completion events and its profiling marks.  What is NOT here is shared by the two groups
 * (scrappie_hip_engine, "shared between the slots"). */
struct Slot {
    LaunchGroup lg;
    bool pending = false;            /* taken: from run_pipeline until scrappie_hip_collect picks the group up */
    /* profiling: events are only RECORDED while a launch group runs (no host synchronisation inside the timed region); elapsed times are
     * read back by resolve_spans after the group's done event */
    hipEvent_t ev[48] = {};
    int nev = 0;                     /* events of ev[] the group has recorded */
    struct Span { int field, i, j; };
    std::vector<Span> spans;
    scrappie_hip_timing timing{};
    hipEvent_t done = nullptr;       /* results are in pinned memory (cstream) */
    hipEvent_t kdone = nullptr;      /* kernels of the slot finished (stream) -> copies may start (cstream) */
    hipEvent_t hdone = nullptr;      /* traceback walk + k_stitch of the slot finished (cstream) */
    hipEvent_t pdone = nullptr;      /* prologue finished (pstream) -> the main stream may go on */
    hipEvent_t up = nullptr;         /* upload into d_signal finished */
    DBuf d_meta, d_signal, d_gflag;
    DBuf d_conv;                     /* convolution output (the layers' ping-pong buffers belong to the group that is running) */
    DBuf d_bad;                      /* [npad]: read whose input left the split products' operand range (k_conv_act, k_feat_in) */
    DBuf d_edge;                     /* k_gru_conv: where each read's convolution windows end (ShConvFuse::edge) */
    DBuf d_fscore, d_seq, d_hp;
    DBuf d_pos, d_bases, d_blen, d_redo;     /* k_stitch: pos / bases / lengths / host-decides flags */
    DBuf d_dwmeta; HBuf h_dwmeta;            /* k_walk_dwell_out: dwell offsets, prior numerators and capacities in tiled order */
    DBuf d_post, d_postoff; HBuf h_post, h_postoff;      /* k_crf_post: the group's base probabilities and their offsets in tiled order */
    hipEvent_t pev[5] = {};          /* ... and its timing marks (sh_eng_crfpost.inc; made on first use) */
    HBuf h_meta, h_sig, h_err, h_bad, h_edge, h_seq, h_score, h_hp, h_pos, h_bases, h_blen, h_redo;
    size_t pinned_bytes() const {
        size_t tot = 0;
        for (const HBuf *h : {&h_meta, &h_sig, &h_err, &h_bad, &h_edge, &h_seq, &h_score, &h_hp, &h_pos, &h_bases, &h_blen, &h_redo, &h_dwmeta, &h_post, &h_postoff}) tot += h->cap;
        return tot;
    }
    bool create_events() {
        bool ok = true;
        for (auto &x : ev) ok &= hipEventCreate(&x) == hipSuccess;
        for (hipEvent_t *x : {&done, &kdone, &hdone, &pdone, &up}) ok &= hipEventCreateWithFlags(x, hipEventDisableTiming) == hipSuccess;
        return ok;
    }
    ~Slot() {      /* (with the engine: its device current, its streams drained) */
        for (auto &x : ev) if (x) (void)hipEventDestroy(x);
        for (auto &x : pev) if (x) (void)hipEventDestroy(x);
        for (hipEvent_t x : {done, kdone, hdone, pdone, up}) if (x) (void)hipEventDestroy(x);
    }
};

/* Caller-supplied data in place of a stage's output (measurement / test hooks, set while nothing is in flight): where each read of a call starts in
 * it, and what its image in a launch group's layout was last built for -- once per launch-group shape (inject_alt, sh_eng_pipeline.inc). */
struct AltInput {
    const float *data = nullptr;
    std::vector<uint64_t> off;
    DBuf d_off;
    uint64_t key = 0; bool valid = false;
    explicit operator bool() const { return data != nullptr; }
    int set(const char *who, const float *d, const uint64_t *o, size_t n) {
        valid = false;
        if (!d) { data = nullptr; off.clear(); return 0; }
        if (!o || n == 0) return set_err("%s: no offsets", who);
        data = d; off.assign(o, o + n);
        return 0;
    }
};

struct scrappie_hip_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t cstream = nullptr;   /* results -> host, so that the copy overlaps the next group's kernels */
    hipStream_t ustream = nullptr;   /* host signals -> device (scrappie_hip_basecall_batch), same reason */
    hipStream_t pstream = nullptr;   /* prologue of a launch group: metadata upload, flag clears, convolution -- runs under the PREVIOUS group's
                                        recurrent layers (k_conv_act fits beside k_gru_proj's waves), the main stream waits for the slot's pdone */
    size_t total_mem = (size_t)64 << 30;
    size_t max_launch_blocks = 0;    /* column blocks (16 reads x 1 block) per launch group; 0 = from device memory */
    std::vector<Model *> models;
    size_t max_launch_reads = 16384;
    bool profiling = false;
    scrappie_hip_timing timing{};
    bool ev_ok = false;
    Slot slots[2];               /* the two launch groups in flight */
    int cur = 0;                 /* slot of the most recent run_pipeline */
    int oldest = 0;              /* next slot collect() will take */
    Slot &current() { return slots[cur]; }
    Slot &other(const Slot &sl) { return slots[&sl == &slots[0] ? 1 : 0]; }
    int index(const Slot &sl) const { return (int)(&sl - slots); }
    bool any_pending() const { return slots[0].pending || slots[1].pending; }
    void drain() {                /* after a failure: nothing left in flight, nothing left to collect */
        (void)sh_stream_wait(pstream); (void)sh_stream_wait(stream); (void)sh_stream_wait(cstream);
        slots[0].pending = slots[1].pending = false;
    }
    /* shared between the slots: the buffers only the kernels of ONE group touch at a time.  The main stream runs the groups' kernels one group
     * after the other, which orders the layers' buffers (d_act[1..2], d_xaff), S1's (d_E, d_sums) and the hand-over state (d_hstate, d_vstate,
     * d_vflag).  The traceback (d_tb, d_tbend, d_fstate) is read by the walk back on the copy stream: a group's decoder waits for the other
     * slot's done event before it overwrites them (run_pipeline).  The alt_* images further down belong to hooks that run with nothing in flight. */
    DBuf d_hstate, d_vstate, d_vflag;
    DBuf d_act[3];                /* ([0] is unused: the convolution's output is the slot's d_conv) */
    DBuf d_xaff, d_E, d_sums, d_tb, d_tbend, d_fstate;
    int ncu = 256;
    bool handover = true;         /* cut tiles between lanes / into pieces (SCRAPPIE_HIP_HANDOVER=0: whole tiles only) */
    AltInput alt_prob; DBuf d_Ealt, d_sums_alt;      /* scrappie_hip_set_decoder_input: probabilities in place of the S1 output, their decoder image */
    AltInput alt_trunk; DBuf d_act_alt;              /* scrappie_hip_set_trunk_input: trunk activations in front of S1, their chunk-layout image */
    /* scrappie_hip_debug_option */
    bool dbg_ff_separate = false;    /* S1 and the decoder as two kernels (as SH_FF_SEPARATE, per engine) */
    bool dbg_fv_single = false;      /* S1 inside the decoder on k_ff_viterbi's eight do-everything waves (as SH_FV_SINGLE, per engine) */
    bool dbg_dump_final = false;     /* decoders leave every tile's final scores in d_vstate */
    int dbg_fail_run = 0;            /* k > 0: the k-th next launch group is refused (failure-path tests) */
    bool dbg_redo_all = false;       /* treat every read as one k_stitch left to the host (tests the fallback) */
    bool dbg_dwell_tight = false;    /* dwell-mode groups reserve 16 bytes of bases a read: longer calls overflow on the device and go to the host (tests that path) */
    int dbg_gru_tiles = 0;           /* 1 / 2: tiles per workgroup of k_gru_proj whatever the schedules say (0: choose) */
    int dbg_decoder_cus = 0;         /* n > 0: the decoder's piece schedule is made for a device of n CUs, so a launch group of a few tiles is cut into pieces (0: the device's own count) */
    int dbg_decoder_lanes = 0;       /* n > 0: the two-team decoder's lane layout is made for a device of n CUs, so a few tiles share n workgroups and are cut between them (0: the device's own count) */
    bool dbg_force_f32 = false;      /* models loaded from now on run their GRU layers on the exact-fp32 kernels (as if out of the split products' range) */
    int dbg_gru32 = -1;              /* 0 / 1: recurrent layers on 16- / 32-read tiles whatever the build's default (-1) */
    /* chain-bound reads beside the rest of a call (scrappie_hip_basecall_batch): a helper engine on the same device, created on first use */
    scrappie_hip_engine *tail = nullptr;
    scrappie_hip_engine *tail2 = nullptr;   /* a second helper, created when a ticket arrives while the first is busy: a chain-bound launch group lasts
                                               as long as its longest read whatever it holds, so a stream of calls with a heavy tail keeps two going */
    bool is_tail = false;
    int tail_mode = -1;              /* 0 / 1: never / whenever the plan says so; -1: SCRAPPIE_HIP_TAIL (default 1) */
    int dbg_fail_tail = 0;           /* k > 0: the helper engine's k-th next launch group is refused (failure-path tests) */
    double mem_frac = 0.7;           /* share of the device's memory a launch group's arena may take; creating the helper engine (the first call with
                                        chain-bound reads) lowers it to 0.45 for good -- the helper takes 0.3 (two helpers: 0.15 each; tail_mem_frac) -- so later calls
                                        cut slightly smaller launch groups whether or not they have a long tail (include/scrappie_hip.h) */
    struct Blob { std::string name; std::vector<unsigned char> bytes; bool force_f32; };
    std::vector<Blob> blobs;         /* the models as they were loaded (replayed into the helper engine) */
    unsigned long long n_tail_calls = 0, n_tail_reads = 0;       /* calls split so far, reads that went to the helper (debug_fetch) */
    /* the helper's host thread: takes ALL waiting tickets of one kind as one launch group -- chain-bound groups last as long as their
     * longest read however many long reads they hold, so the long reads of several calls cost what those of one call cost */
    struct TailTicket {
        long id = 0; int model = 0; scrappie_hip_params p{};
        std::vector<raw_table> reads; std::vector<scrappie_hip_call> calls;
        std::vector<float> own;          /* device-resident callers: the deferred reads' signals, copied back so that they outlive the caller's buffer */
        int rc = 0; std::string err; bool done = false;
    };
    std::thread tail_th, tail_th2;
    bool tail_th_live = false, tail_th2_live = false, tail_stop = false;
    int tail_busy = 0;                       /* helpers with a launch group in hand */
    std::mutex tail_mu;
    std::condition_variable tail_cv;
    std::deque<std::shared_ptr<TailTicket>> tail_q;
    std::map<long, std::shared_ptr<TailTicket>> tail_open;
    long tail_next = 1;
    unsigned long long n_redo_tail = 0;      /* reads the helper's k_stitch left to the host */
    unsigned long long n_tail_groups = 0;    /* launch-group calls the helper has made (fewer than tickets when tickets were merged) */
    unsigned host_thread_budget = 0; /* stitching threads of this engine while several engines share a call (0: host_threads()) */
    unsigned long long n_redo = 0;   /* reads k_stitch left to the host so far (scrappie_hip_debug_fetch "n_redo") */
    /* scrappie_hip_basecall_device_stream: the last launch group of the previous call, still in flight */
    struct Carry { bool live = false; int slot = 0; std::vector<uint32_t> perm; scrappie_hip_call *out = nullptr; scrappie_hip_params p{}; } carry;
    std::mutex mu;
    double tail_frac = 0.3;          /* the helper engine's share of the device's memory as settled when it was made (free memory then, at most tail_mem_frac()) */
    double dbg_tail_free_frac = 0;   /* test hook (debug option "tail_free_frac", in 1/1000): the free share the helper's creation sees */
    BatchCoalescer batch_co;         /* this engine's queue of small scrappie_hip_basecall_batch calls, and the threads seen inside them lately */
    ShPresence batch_presence;
    /* staging of the per-read functions (sh_eng_surface.inc), touched under mu only (a PostStage's pinned half: see above), grow-only and kept between
     * calls.  They belong to the engine, not to the queue in front of it: a call with the queue off, or on an engine of its own, runs the same batch
     * functions with nobody but mu to keep two callers apart. */
    PostStage post_stage[2]; unsigned post_turn = 0;     /* posterior_batch: two in turn, so that a batch seldom waits for the last one's callers */
    HBuf h_dec_in, h_dec_out; DBuf d_dec[7];             /* decode_batch: posteriors in (a lone call; the queue's members fill the queue's own), paths + scores out */
    HBuf h_crf_in, h_crf_out; DBuf d_crf[4];             /* crf_batch */
    DpBufs dp_map; DBuf d_map_seq, d_map_band, d_map_post;       /* block-based mapping (sh_eng_map.inc): the records' buffers; codes, bands, a per-read call's dense posterior */
    PackState map_pack, map_crf_pack;      /* candidates in packs, of transducer reads (k_map_pack) and of flip-flop reads (k_map_crf_pack): sh_eng_cands.inc */
    DpBufs dp_mcl; DBuf d_mcl_seq, d_mcl_first;      /* sequence-local CRF mapping (sh_eng_map_crf_local.inc): the windows' buffers (final state: the end cell, an int2); codes, the second pass's firsts */
    DpBufs dp_ml; DBuf d_ml_seq, d_ml_lohi;      /* sequence-local transducer mapping (sh_eng_map_local.inc): the windows' buffers (final state: the end position and kind, an int2); codes, the second pass's (first, last) */
    int map_local_stride = -1;       /* entry positions a window of k_map_local owns (debug option "map_local_stride"; 0: one window, -1: the default) */
    DBuf d_cfd_rd, d_cfd_cell, d_cfd_score, d_cfd_pos, d_cfd_call; HBuf h_cfd;      /* motifs searched inside flip-flop reads (sh_eng_crf_find.inc): the packs, their cell words, scores, (begin, end), call scores; results on the host */
    int crf_find_cells = -1;         /* cells a pack of motifs holds (debug option "crf_find_cells"; -1: the default) */
    EditsState crf_edits, map_edits; /* every single-base edit of a sequence against a flip-flop read and against a transducer read (sh_eng_edits.inc): one each, so that either family's timing outlives the other's calls */
    int map_edits_band_width = 0;    /* positions per workgroup of the banded k_map_edits: 64 or 256; 0: the default of the form (debug option "map_edits_band_width") */
    int map_crf_local_stride = -1;   /* start cells a window of k_map_crf_local owns (debug option "map_crf_local_stride"; 0: one window, -1: the default) */
    double map_ms[3] = {0, 0, 0};    /* scrappie_hip_map_batch: network + S1, k_map, k_map_walk + results, summed over the last call's launch groups */
    DpBufs dp_sq; DBuf d_sq_sig, d_sq_tab;       /* squiggle matching (sh_eng_squig.inc): the records' buffers; signals, tables */
    DBuf d_sqp_rd, d_sqp_sig, d_sqp_w, d_sqp_score; HBuf h_sqp;      /* candidate squiggles in packs (sh_eng_squig_pack.inc): the packs, the reads' signals, the packs' tables and words, scores; signals and scores on the host */
    bool squig_pack_lone = false;    /* a candidate alone in its pack runs in k_squig_pack all the same (debug option "squig_pack_lone"; default: it takes k_squig) */
    int squig_pack_cells = -1;       /* cells a pack of candidate squiggles holds (debug option "squig_pack_cells"; 0: every candidate through k_squig, -1: the default) */
    DpBufs dp_sql; DBuf d_sql_sig, d_sql_tab, d_sql_lohi; HBuf h_sql;      /* reference-local squiggle mapping (sh_eng_squig_local.inc): the windows' buffers (final state: the end position and kind, an int2); signals, tables, the second pass's (first, last); signals on the host */
    int squig_local_stride = -1;     /* entry positions a window of k_squig_local owns (debug option "squig_local_stride"; 0: one window, -1: the default) */
    double squig_ms[3] = {0, 0, 0};  /* scrappie_hip_squiggle_match_batch: tables + uploads, k_squig, k_squig_walk + results, summed over the last call's launches */
    DBuf d_sqn[2]; HBuf h_sqn;       /* squiggle prediction (sh_eng_sqnet.inc): tiles | codes, outputs */
    double sqnet_ms[3] = {0, 0, 0};  /* scrappie_hip_squiggle_predict_batch: upload, k_sqnet, download + transform, summed over the last call's launches */
    DBuf d_ev_sig, d_ev_rd, d_ev_sum, d_ev_sumsq, d_ev_t1, d_ev_t2, d_ev_peaks, d_ev_np, d_ev_off, d_ev_out; HBuf h_ev, h_ev_out;      /* event detection (sh_eng_events.inc): signals, records, the five scratch arrays, peak counts, event offsets, event tables; staging */
    double event_ms[3] = {0, 0, 0};  /* scrappie_hip_detect_events_batch: staging + upload, the kernels, tables to the host, summed over the last call's launches */
    HBuf h_cp_in, h_cp_out; DBuf d_cp_in, d_cp_out;      /* scrappie_hip_posterior_crf_batch (sh_eng_crfpost.inc): matrices + per-read words, probabilities */
    double crf_post_ms[3] = {0, 0, 0};   /* scrappie_hip_crf_post_timing: the last call's three terms, summed over its launch groups */
    size_t dbg_events_budget = 0;    /* sample slots one event-detection launch may hold (debug option "events_budget_samples"; 0: from the free memory) */
    size_t dbg_sqnet_budget = 0;     /* device bytes one squiggle-predicting launch may hold (debug option "sqnet_budget_kb"; 0: half of the free memory) */
    size_t dbg_squig_budget = 0;     /* device bytes one squiggle-matching launch may hold (debug option "squiggle_budget_kb"; 0: half of the free memory) */
    std::mutex call_mu;              /* scrappie_hip_basecall_batch: one call at a time inside the engine (concurrent small calls share one: sh_eng_batch.inc) */
    /* (scrappie_hip_engine_destroy has made the device current and drained the streams; the slots and the buffers go after this body) */
    ~scrappie_hip_engine() {
        for (Model *m : models) delete m;
        for (hipStream_t st : {stream, cstream, ustream, pstream}) if (st) (void)hipStreamDestroy(st);
    }
};

static int pick_mt(int mtiles) {
    for (int mt : {6, 4, 3, 2}) if (mtiles % mt == 0) return mt;
    return 1;
}

/* HIP gives a process 4 hardware queues by default and maps its streams onto them round robin.  An engine owns 4
 * streams (main, prologue, helpers, upload); with anybody else's streams in the process (the null stream, torch,
 * RCCL, a second engine) two of them share a queue and work that is meant to overlap serialises (bench.py under a
 * process group: 29.7 against 28.2 ms per step; two engines on one device: no overlap at all, profiles/r3_long_tail.txt).
 * GPU_MAX_HW_QUEUES is read when the HIP runtime initialises, so this default only takes effect if the library makes the
 * process's first HIP call; a host that has HIP running already sets the variable itself.  Never
 * overrides a value the user has set. */
static void hw_queue_default() {
    static std::once_flag once;
    std::call_once(once, [] { (void)setenv("GPU_MAX_HW_QUEUES", "8", 0); });
}

static int device_count(hipError_t *why) {
    hw_queue_default();
    int n = 0;
    const hipError_t rc = hipGetDeviceCount(&n);
    if (why) *why = rc;
    return rc == hipSuccess ? n : 0;
}
extern "C" int scrappie_hip_device_count(void) { return device_count(nullptr); }
/* the NUMA node a device's PCIe root belongs to (-1: unknown / one node): where its engine's and preparer's pinned buffers are placed (sh_numa.h) */
extern "C" int scrappie_hip_device_numa_node(int device) { return sh_device_numa_node(device); }

extern "C" scrappie_hip_engine *scrappie_hip_engine_create(int device) {
    hipError_t why = hipSuccess;
    int n = device_count(&why);
    if (n <= 0) {
        /* the usual reason on a box that has a GPU: two copies of the HIP runtime in one process (a torch wheel's own next to
         * /opt/rocm's) -- the one that initialises second finds no device */
        std::string first, second;
        if (FILE *maps = fopen("/proc/self/maps", "r")) {
            char line[1024];
            while (fgets(line, sizeof line, maps)) {
                const char *path = strchr(line, '/');
                if (!path || !strstr(path, "libamdhip64")) continue;
                std::string s(path, strcspn(path, "\n"));
                if (first.empty()) first = s; else if (s != first && second.empty()) second = s;
            }
            fclose(maps);
        }
        if (!second.empty())
            set_err("no HIP device visible (hipGetDeviceCount: %s): two HIP runtimes are loaded in this process (%s and %s); load the "
                    "other user of HIP (e.g. import torch) before this library, see INTEGRATION.md", hipGetErrorString(why), first.c_str(), second.c_str());
        else set_err("no HIP device visible (hipGetDeviceCount: %s)", hipGetErrorString(why));
        return nullptr;
    }
    if (device < 0 || device >= n) { set_err("device %d out of range (have %d)", device, n); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { set_err("hipSetDevice(%d) failed", device); return nullptr; }
    hipDeviceProp_t prop;
    int ncu = 256;
    size_t total_mem = (size_t)64 << 30;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        if (prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
        if (prop.totalGlobalMem > 0) total_mem = prop.totalGlobalMem;
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            set_err("device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
            return nullptr;
        }
    }
    (void)tun();                                   /* development switches: environment read here, once */
    scrappie_hip_engine *e = new scrappie_hip_engine();
    e->device = device;
    e->ncu = ncu;
    e->total_mem = total_mem;
    { const char *h = getenv("SCRAPPIE_HIP_HANDOVER"); if (h && atoi(h) == 0) e->handover = false; }
    /* the main stream at the highest priority: where a helper kernel and a recurrent layer compete for a CU, the layer goes first */
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
#ifdef SH_EXPERIMENTS
    if (!getenv("SH_STREAM_PRIO"))
#endif
    prio_lo = prio_hi = 0;      /* experiment switch: stream priorities off unless asked for */
    if (hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipStreamCreateWithPriority(&e->cstream, hipStreamNonBlocking, prio_lo) != hipSuccess ||
        hipStreamCreateWithPriority(&e->pstream, hipStreamNonBlocking, prio_lo) != hipSuccess ||
        hipStreamCreateWithFlags(&e->ustream, hipStreamNonBlocking) != hipSuccess) {
        set_err("hipStreamCreate failed");
        delete e;
        return nullptr;
    }
    e->ev_ok = true;
    for (Slot &sl : e->slots) if (!sl.create_events()) e->ev_ok = false;
    return e;
}

extern "C" void scrappie_hip_engine_destroy(scrappie_hip_engine *e) {
    if (!e) return;
    if (e->tail_th_live) {
        { std::lock_guard<std::mutex> lk(e->tail_mu); e->tail_stop = true; }
        e->tail_cv.notify_all();
        e->tail_th.join();
        e->tail_th_live = false;
        if (e->tail_th2_live) { e->tail_th2.join(); e->tail_th2_live = false; }
    }
    for (auto &kv : e->tail_open) if (kv.second->done && !kv.second->rc) scrappie_hip_free_calls(kv.second->calls.data(), kv.second->calls.size());     /* never collected */
    e->tail_open.clear();
    if (e->tail) { scrappie_hip_engine_destroy(e->tail); e->tail = nullptr; }
    if (e->tail2) { scrappie_hip_engine_destroy(e->tail2); e->tail2 = nullptr; }
    (void)hipSetDevice(e->device);
    for (hipStream_t st : {e->stream, e->cstream, e->ustream, e->pstream}) if (st) (void)sh_stream_wait(st);
    delete e;      /* (events, streams, models and every buffer: ~scrappie_hip_engine, ~Slot, ~DBuf / ~HBuf) */
}

extern "C" scrappie_hip_params scrappie_hip_default_params(void) {
    scrappie_hip_params p;
    p.min_prob = 1e-5f; p.tempW = 1.0f; p.tempb = 1.0f;
    p.stay_pen = 0.0f; p.skip_pen = 0.0f; p.local_pen = 2.0f;
    p.use_slip = 0; p.homopolymer = HOMOPOLYMER_MEAN; p.want_pos = 0;
    return p;
}

#include "sh_eng_load.inc"      /* the .scrm container -> Model, engine settings, the planning functions of the ABI */
#include "sh_eng_launch.inc"      /* launch-group construction (tiles, metadata, schedules) and the kernel dispatch helpers */
#include "sh_eng_pipeline.inc"      /* run_pipeline: one launch group through its kernels, a function per stage */
#include "sh_eng_groups.inc"      /* run_device / collect / stitching, a call cut into launch groups, device-resident entry points */
#include "sh_eng_batch.inc"      /* chain-bound reads on a helper engine, host-signal entry points, several GPUs */
#include "sh_eng_debug.inc"      /* measurement / test hooks: decoder and trunk inputs, debug_option / debug_fetch / debug_stitch */
#include "sh_eng_surface.inc"      /* the reference's per-read functions: posterior / trunk on an explicit engine, the process-default engine, decode_transducer, decode_crf; all three coalesced (sh_coalesce.h) */
#include "sh_eng_cut.inc"      /* shared by those below: LaunchCut (a call cut into launches), dp_order / dp_launch / dp_collect (a kernel with two homes) */
#include "sh_eng_post.inc"      /* shared by the mapping engines below: PostCall (the batch call), post_group (a launch group to STOP_POST), DpPlan / dp_run, PackSet / PackLaunch, post_upload_* */
#include "sh_eng_win.inc"      /* shared by the three reference-local engines below: WinCut / win_cut, WinTraits, win_launch / win_run, win_lse, win_read_bytes; seq_win_run / seq_win_batch for the two map families */
#include "sh_eng_map_crf.inc"      /* mapping of flip-flop reads to base sequences (sh_map_crf.h): map_crf_to_sequence_* on the process-default engine, the launch group scrappie_hip_map_batch runs for a CRF model */
#include "sh_eng_map.inc"      /* block-based mapping (sh_map.h): map_to_sequence_* on the process-default engine, scrappie_hip_map_batch */
#include "sh_eng_cands.inc"      /* shared by the two below: CandTraits, CandSet / cand_set_build, CandJob, cand_run, cand_one, cand_group / cand_batch, scrappie_hip_free_map_multi_results */
#include "sh_eng_map_pack.inc"      /* one read against many candidate sequences (sh_map_pack.h): scrappie_hip_map_multi_batch, scrappie_hip_map_post_multi */
#include "sh_eng_map_crf_pack.inc"      /* one flip-flop read against many candidate sequences (sh_map_crf_pack.h): scrappie_hip_map_crf_multi_batch, scrappie_hip_map_trans_multi */
#include "sh_eng_edits.inc"      /* shared by the two below: EditsTraits, EditsJob, edits_launch / edits_run, edits_one, edits_batch, scrappie_hip_free_edits_results */
#include "sh_eng_crf_edits.inc"      /* every single-base edit of a sequence against a flip-flop read (sh_crf_edits.h): scrappie_hip_map_crf_edits_batch, map_crf_edits */
#include "sh_eng_map_edits.inc"      /* every single-base edit of a sequence against a transducer read (sh_map_edits.h): scrappie_hip_map_edits_batch, map_post_edits */
#include "sh_eng_crf_find.inc"      /* short sequences searched inside flip-flop reads, packed into workgroups (sh_crf_find.h): find_crf_sequences_viterbi, scrappie_hip_find_batch */
#include "sh_eng_map_crf_local.inc"      /* flip-flop reads mapped into a longer sequence, cut into windows (sh_map_crf_local.h): map_crf_to_reference_*, scrappie_hip_map_local_batch */
#include "sh_eng_map_local.inc"      /* transducer reads mapped into a longer sequence, cut into windows (sh_map_local.h): map_to_reference_*, scrappie_hip_map_post_local_batch */
#include "sh_eng_squig.inc"      /* squiggle matching (sh_squig.h): squiggle_match_* on the process-default engine, scrappie_hip_squiggle_match_batch */
#include "sh_eng_squig_pack.inc"      /* one signal against many candidate squiggles (sh_squig_pack.h): scrappie_hip_squiggle_match_multi_batch, scrappie_hip_squiggle_match_multi */
#include "sh_eng_squig_local.inc"      /* raw signals mapped into a longer reference squiggle, cut into windows (sh_squig_local.h): squiggle_match_local_*, scrappie_hip_squiggle_match_local_batch */
#include "sh_eng_sqnet.inc"      /* squiggle prediction (sh_sqnet.h): squiggle_r94 and its relatives on the process-default engine, scrappie_hip_squiggle_predict_batch */
#include "sh_eng_events.inc"      /* event detection (sh_events.h): detect_events on the process-default engine, scrappie_hip_detect_events_batch; `scrappie events` for a batch (scrappie_hip_basecall_events_batch) */
#include "sh_eng_crfpost.inc"      /* base probabilities of the flip-flop models (sh_crf_post.h): scrappie_hip_basecall_batch_probs, scrappie_hip_posterior_crf_batch */
