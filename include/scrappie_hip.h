/* include/scrappie_hip.h -- C ABI of libscrappie_hip.so, the MI355X-native
 * implementation of the `scrappie raw` basecalling hot path.
 *
 * Two surfaces:
 *
 *  (1) The reference's per-read surface, same names, signatures, struct
 *      layouts, ownership and NULL/NAN-on-error behaviour, so that a binding
 *      written against the reference (python/pyscrap.h, interface/scrappie.h,
 *      src/decode.h, src/networks.h) loads this library unchanged.  Each
 *      declaration cites the reference prototype it replaces.
 *
 *  (2) An additive batched engine surface (the reference has none: it calls
 *      one read at a time, src/scrappie_raw.c:265).  This is the fast path:
 *      reads are coalesced into launch groups that fill the GPU, decoded on
 *      device, and only paths/bases return over PCIe.
 *
 * Plain C types only: no torch, no HIP types.  Device pointers cross the
 * boundary as `void *` / `const float *` and are documented as such.
 */
#ifndef SCRAPPIE_HIP_H
#define SCRAPPIE_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * Types shared with the reference (layouts are ABI)
 * ---------------------------------------------------------------------- */

/* src/scrappie_structures.h:24-30 == interface/scrappie.h:29-35 */
typedef struct {
    char *uuid;
    size_t n;
    size_t start;
    size_t end;
    float *raw;
} raw_table;

/* src/scrappie_structures.h:8-22 (events basecaller input) */
typedef struct {
    uint64_t start;
    float length;
    float mean;
    float stdv;
    int pos;
    int state;
} event_t;

typedef struct {
    size_t n;
    size_t start;
    size_t end;
    event_t *event;
} event_table;

/* src/event_detection.h:6-21 */
typedef struct {
    size_t window_length1;
    size_t window_length2;
    float threshold1;
    float threshold2;
    float peak_height;
} detector_param;
extern const detector_param event_detection_defaults;      /* 3, 6, 1.4, 9.0, 0.2 */

/* src/scrappie_matrix.h:10-16 == interface/scrappie.h:38-45.  Column-major,
 * rows padded to nrq = ceil(nr/4) 4-float vectors, stride = 4*nrq, 16-byte
 * aligned.  The `v` arm is `__m128 *` in the reference; any object pointer
 * keeps the layout. */
typedef struct {
    size_t nr, nrq, nc, stride;
    union {
        void *v;
        float *f;
    } data;
} _Mat;
typedef _Mat *scrappie_matrix;
typedef _Mat const *const_scrappie_matrix;

/* src/networks.h:8-14 */
enum raw_model_type {
    SCRAPPIE_MODEL_RAW = 0,
    SCRAPPIE_MODEL_RGRGR_R9_4,
    SCRAPPIE_MODEL_RGRGR_R9_4_1,
    SCRAPPIE_MODEL_RGRGR_R10,
    SCRAPPIE_MODEL_RNNRF_R9_4,
    SCRAPPIE_MODEL_INVALID
};

/* src/homopolymer.h */
enum homopolymer_calculation {
    HOMOPOLYMER_NOCHANGE = 0,
    HOMOPOLYMER_MEAN,
    HOMOPOLYMER_INVALID
};

/* src/networks.h:22 */
typedef scrappie_matrix (*posterior_function_ptr)(const raw_table, float, float, float, bool);

/* ------------------------------------------------------------------------
 * (1) Per-read surface -- drop-in for the reference symbols
 * ---------------------------------------------------------------------- */

/* src/networks.c:17, :49, :87, :108 */
enum raw_model_type get_raw_model(const char *modelstr);
const char *raw_model_string(const enum raw_model_type model);
int get_raw_model_stride(const enum raw_model_type model);
posterior_function_ptr get_posterior_function(const enum raw_model_type model);
/* python/build.py:34-44 (defined only in the cffi build of the reference) */
int get_raw_model_stride_from_string(const char *modelstr);

/* src/networks.c:250, :299, :348, :567 (python/pyscrap.h:11-23).  Run on the
 * process-default engine (device 0 or $SCRAPPIE_HIP_DEVICE) as a launch group
 * of one read; the returned matrix is HOST memory in the reference's padded
 * layout, released with free_scrappie_matrix.  NULL on any failure.  Weights
 * come from the model registered under the same name (scrappie_hip_register_
 * model / $SCRAPPIE_MODEL_DIR/<name>.scrm); the reference compiles them in. */
/* src/networks.c:196 (interface/scrappie.h:49): bi-GRU model raw_r94 */
scrappie_matrix nanonet_raw_posterior(const raw_table signal, float min_prob,
                                      float tempW, float tempb, bool return_log);
scrappie_matrix nanonet_rgrgr_r94_posterior(const raw_table signal, float min_prob,
                                            float tempW, float tempb, bool return_log);
scrappie_matrix nanonet_rgrgr_r941_posterior(const raw_table signal, float min_prob,
                                             float tempW, float tempb, bool return_log);
scrappie_matrix nanonet_rgrgr_r10_posterior(const raw_table signal, float min_prob,
                                            float tempW, float tempb, bool return_log);
scrappie_matrix nanonet_rnnrf_r94_transitions(const raw_table signal, float min_prob,
                                              float tempW, float tempb, bool return_log);
/* src/networks.c:146: events bi-LSTM; weights from the model registered as
 * "nanonet_events".  Features (nnfeatures.c:88, Kahan studentisation with rsqrtps) and the
 * 3-event window (layers.c:119, first column zero as in the reference) are host C. */
scrappie_matrix nanonet_posterior(const event_table events, float min_prob,
                                  float tempW, float tempb, bool return_log);

/* src/event_detection.c:268 -- events of rt.raw[rt.start .. rt.end): pos = state = -1, start = 0, end = n, .event malloc'd (the caller
 * frees it).  Runs on the process-default engine as a batch of one (sh_events.h); the table is bit-identical to the reference's.  Where the
 * reference is undefined -- no peak in the read, so that create_events reads peaks[-1]: fewer than 2 * window_length2 samples, a constant
 * signal -- and for a NULL or empty signal, or when no engine can be made, the result is {0, 0, 0, NULL} and
 * scrappie_hip_last_error() says why. */
event_table detect_events(raw_table const rt, detector_param const edparam);

/* src/decode.c:123 -- seq has nblock+1 entries.  Returns NAN on failure. */
float decode_transducer(const_scrappie_matrix logpost, float stay_pen, float skip_pen,
                        float local_pen, int *seq, bool allow_slip);
/* src/decode.c:449 -- calloc'd string, caller frees; NULL if every entry is a stay */
char *overlapper(const int *seq, size_t n, int nkmer, int *pos);
/* src/decode.h:8-19, src/decode.c:516, :645 -- the dwell correction of homopolymer lengths, the last step of `scrappie events`: host C
 * (sh_host.c), what the device form (sh_dwell.h) is held against.  seq and dwell have n entries; et.event[et.start .. et.end) carry
 * pos (overlapper's) and state (1 + seq) as scrappie_events.c:308-311 sets them; basecall_len is the strlen of the plain overlapper
 * call.  calloc'd strings as strlen sees the reference's (a call that ends inside a homopolymer ends one base short of its length,
 * decode.c:633-635), the caller frees; NULL where the reference is undefined: no k-mer in seq, a homopolymer count that is no int. */
typedef struct {
    float scale;
    float base_adj[4];
} dwell_model;
char *dwell_corrected_overlapper(const int *seq, const int *dwell, int n, int nkmer, const dwell_model dm);
char *homopolymer_dwell_correction(const event_table et, const int *seq, size_t nstate, size_t basecall_len);
/* the homo_scale homopolymer_dwell_correction uses (decode.c:666-693), NAN for an empty table */
float scrappie_hip_dwell_scale(const event_table et, size_t basecall_len);
/* src/decode.c:836, :895, :928 */
float decode_crf(const_scrappie_matrix trans, int *path);
char *crfpath_to_basecall(int const *path, size_t npos, int *pos);
scrappie_matrix posterior_crf(const_scrappie_matrix trans);
/* src/homopolymer.c:175 */
int homopolymer_path(const_scrappie_matrix post, int *viterbipath,
                     enum homopolymer_calculation pathCalculationFlag);

/* src/util.c:190, src/scrappie_common.c:5, :39 */
void medmad_normalise_array(float *x, size_t n);
raw_table trim_and_segment_raw(raw_table rt, size_t trim_start, size_t trim_end,
                               size_t varseg_chunk, float varseg_thresh);
raw_table trim_raw_by_mad(raw_table rt, size_t chunk_size, float perc);

/* src/scrappie_matrix.c:11, :69, :130 */
scrappie_matrix make_scrappie_matrix(size_t nr, size_t nc);
scrappie_matrix mat_from_array(const float *x, size_t nr, size_t nc);
scrappie_matrix free_scrappie_matrix(scrappie_matrix mat);

/* Block-based mapping of a transducer log-posterior to a sequence (src/decode.c:1420, :1547, :1638, :1706, :1844;
 * python/pyscrap.h:41-58).  Same signatures and NULL/NAN conventions; the DP runs on the process-default engine (one
 * launch per call: calls from several threads serialise on the engine).  Viterbi scores and paths are bit-identical to
 * the reference's; forward agrees to float rounding.  Where the reference is undefined (seqlen == 0, a seq
 * code outside [0, nr - 1), a banded call with seqlen < 3, a posterior of no blocks, seqlen above 65536) these return NAN
 * and set scrappie_hip_last_error().  path: nblock int32 positions, -1 in START / END (decode.c:1519-1523). */
bool are_bounds_sane(size_t const *low, size_t const *high, size_t nblock, size_t seqlen);
float map_to_sequence_forward(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                              int const *seq, size_t seqlen);
float map_to_sequence_forward_banded(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                     int const *seq, size_t seqlen, size_t const *poslow, size_t const *poshigh);
float map_to_sequence_viterbi(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                              int const *seq, size_t seqlen, int *path);
float map_to_sequence_viterbi_banded(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                     int const *seq, size_t seqlen, size_t const *poslow, size_t const *poshigh);
/* src/scrappie_seq_helpers.c:53 (python/pyscrap.h:61): n - state_len + 1 codes, calloc'd; NULL on a base outside
 * ACGT/acgt and (the reference is undefined there) when n < state_len */
int *encode_bases_to_integers(char const *seq, size_t n, size_t state_len);

/* Mapping of a raw signal to a predicted squiggle (src/decode.c:1035, :1262; python/pyscrap.h:33-39).  Same signatures; the
 * dynamic programme runs on the process-default engine as a batch of one (sh_squig.h; calls from several threads
 * serialise on the engine).  params: the reference's predicted squiggle, nc = npos columns of (mean, log sd, dwell logit).
 * signal: trimmed and normalised, mapped over [start, end); path_padded: signal.n int32, -1 outside [start, end) and in
 * the START / END states, positions elsewhere.  The Viterbi score and path are bit-identical to the reference's; forward
 * agrees to float rounding.  Where the reference asserts or is undefined (rate <= 0, prob_back outside [0, 1],
 * start >= end, end > n, a squiggle of no positions, NULL arguments) these return NAN, set scrappie_hip_last_error() and
 * launch nothing.  The squiggle comes from squiggle_r94 and its relatives below, or from anywhere else. */
float squiggle_match_viterbi(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                             float skip_pen, float minscore, int32_t *path_padded);
float squiggle_match_forward(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                             float skip_pen, float minscore);
/* The same inside a band (not in the reference; sh_squig_band.h): low[t], one int32 per sample of the window [start, end), is the
 * first position sample t may map to and width how many: positions [low[t], min(low[t] + width, npos)).  After each sample every
 * position and back state outside its band holds -1e30, nothing else changes: a band of low = 0 and width = npos, and any band
 * that contains the unbanded Viterbi path, give the unbanded score and path bit for bit.  low NULL and width 0: unbanded.  A band
 * that is not valid (0 <= low[t] <= npos - 1, low non-decreasing, width >= 1) or admits no path: NAN and an error text. */
float squiggle_match_viterbi_banded(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                    float skip_pen, float minscore, const int32_t *low, size_t width, int32_t *path_padded);
float squiggle_match_forward_banded(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                    float skip_pen, float minscore, const int32_t *low, size_t width);

/* Prediction of a squiggle from a base sequence (src/networks.c:397, :454, :511; python/pyscrap.h:29-31).  Same signatures:
 * sequence holds n bases coded 0..3 (encode_bases_to_integers(seq, n, 1)); the result has n columns of (mean, log sd, dwell
 * logit), nr 3, stride 4, pad lane 0, malloc'd, freed by free_scrappie_matrix.  transform_units: column 1 <- expf(x),
 * column 2 <- expf(-x), on the host with libm.  The network (an embedding and six convolutions, sh_sqnet.h) runs on the
 * process-default engine as a batch of one; its weights are the model registered under the function's name
 * (scrappie_hip_register_model, or <name>.scrm under SCRAPPIE_MODEL_DIR).  The output agrees with the reference's to float
 * rounding (another summation order).  Where the reference is undefined or asserts (a NULL sequence, fewer than WL - 1
 * bases -- WL 9, for squiggle_r94_rna 7: the edge products of `convolution` read outside their input --, a code outside
 * 0..3) and for an unregistered model these return NULL, set scrappie_hip_last_error() and launch nothing. */
scrappie_matrix squiggle_r94(int const *sequence, size_t n, bool transform_units);
scrappie_matrix squiggle_r94_rna(int const *sequence, size_t n, bool transform_units);
scrappie_matrix squiggle_r10(int const *sequence, size_t n, bool transform_units);

/* ------------------------------------------------------------------------
 * (2) Batched engine surface (additive)
 * ---------------------------------------------------------------------- */

typedef struct scrappie_hip_engine scrappie_hip_engine;

/* Decode / posterior parameters: defaults are the CLI's, src/scrappie_raw.c:98-121 */
typedef struct {
    float min_prob;      /* -m   1e-5 */
    float tempW;         /* --temperature1 1.0 */
    float tempb;         /* --temperature2 1.0 */
    float stay_pen;      /* -y   0.0 */
    float skip_pen;      /* -s   0.0 */
    float local_pen;     /* --local 2.0 */
    int use_slip;        /* --slip  0 */
    int homopolymer;     /* enum homopolymer_calculation: HOMOPOLYMER_MEAN */
    int want_pos;        /* fill scrappie_hip_call.pos */
} scrappie_hip_params;

/* One basecall, as struct _raw_basecall_info (src/scrappie_raw.c:25-34) */
typedef struct {
    float score;         /* Viterbi score; NAN if the read produced no call */
    size_t nblock;
    char *basecall;      /* malloc'd, NUL terminated; NULL if no call */
    size_t basecall_length;
    int *pos;            /* malloc'd nblock+1 if want_pos, else NULL */
} scrappie_hip_call;

/* Per-stage device time of the last launch group, milliseconds, measured with
 * HIP events on the engine's own stream (only filled when profiling is on). */
typedef struct {
    float conv_ms, affine_ms, gru_ms, ff_ms, decode_ms, backtrace_ms, total_ms;
    int n_gru_launches, n_affine_launches;
    double gru_flops, affine_flops, ff_flops;   /* algorithmic FLOPs of those launches */
    /* of which: recurrent layers run as one kernel, projection + recurrence (their time is part of
     * gru_ms, their FLOPs = projection + recurrence, counted in affine_flops / gru_flops) */
    float fused_ms;
    int n_fused_launches;
    double fused_flops;
    float stitch_ms;     /* the copy-stream kernel behind the decoder (under the next group): k_walk_stitch_out -- traceback walk + homopolymer correction +
                          * k-mer stitching + results to pinned host memory -- and backtrace_ms is 0; with SH_SPLIT_TAIL=1, host stitching or the flip-flop
                          * models: k_stitch alone, the walk in backtrace_ms */
} scrappie_hip_timing;

int scrappie_hip_device_count(void);
/* NUMA node of the socket the device hangs off (sysfs; -1 when unknown or the host has one node).  Pinned staging and result buffers of the
 * device's engine / preparer are allocated with the calling thread bound to that node's CPUs for the duration of the allocation, so that
 * loader threads write and the GPU's DMA reads socket-local memory on a two-socket node (SCRAPPIE_HIP_NUMA=0: off). */
int scrappie_hip_device_numa_node(int device);
/* last error message of the calling thread ("" if none) */
const char *scrappie_hip_last_error(void);

scrappie_hip_engine *scrappie_hip_engine_create(int device);
void scrappie_hip_engine_destroy(scrappie_hip_engine *e);
scrappie_hip_params scrappie_hip_default_params(void);

/* Load a `.scrm` weight container (scrappie_amd/model.py) and bind it to a
 * reference model name ("raw_r94", "rgrgr_r94", "rgrgr_r941", "rgrgr_r10", "rnnrf_r94").
 * Returns a model handle >= 0, or -1. */
int scrappie_hip_load_model(scrappie_hip_engine *e, const char *name, const char *path);
/* Same from memory: `blob` is the container image. */
int scrappie_hip_load_model_mem(scrappie_hip_engine *e, const char *name,
                                const void *blob, size_t nbytes);
int scrappie_hip_find_model(scrappie_hip_engine *e, const char *name);
/* bind a model to the process-default engine used by the per-read surface */
int scrappie_hip_register_model(const char *name, const char *path);
/* The per-read network functions above may be called from many host threads at once, as the reference's OpenMP loop over reads does
 * (scrappie_raw.c:355,387): calls that arrive while the device is busy, or while the leader waits for company -- windows of SCRAPPIE_HIP_COALESCE_US (default 500)
 * microseconds until three quarters of the threads seen lately have joined or a window passes with no arrival, SCRAPPIE_HIP_COALESCE_MAX_US
 * (default 10000) in all (scrappie_amd/csrc/sh_coalesce.h) -- run as ONE launch group and every caller gets its own matrix -- bit for bit the one it would get alone.  SCRAPPIE_HIP_COALESCE=0: no
 * queue -- one read per launch, calls serialised on the engine (the same code with a batch of one; so is a call on an explicit engine).  out[0..2] = launch groups run this way, reads in them, the largest group (tests, tools). */
void scrappie_hip_coalescer_stats(unsigned long long out[3]);
/* decode_transducer is coalesced the same way (one workgroup per waiting call, as for a call alone: same path, same score) */
void scrappie_hip_decode_coalescer_stats(unsigned long long out[3]);
/* ... and decode_crf (a thread per waiting call) */
void scrappie_hip_crf_coalescer_stats(unsigned long long out[3]);

/* Basecall n reads.  Each raw_table's raw[start..end) must already be trimmed
 * and normalised (as calculate_post does before the network,
 * src/scrappie_raw.c:273-277).  Reads shorter than the model's minimum
 * (scrappie_hip_min_samples) yield no call.  out[i] corresponds to reads[i].
 * Returns 0, or -1 with scrappie_hip_last_error().
 * May be called from several host threads on one engine (round 6): calls of fewer than 4096 reads that are waiting for the same
 * engine, model and parameters run as ONE engine call and share its launch groups -- the reference's `schedule(dynamic)` loop
 * (src/scrappie_raw.c:355,387) with a body that hands over 64 reads at a time keeps the device full that way; every caller gets exactly the
 * calls it would get alone.  Larger calls go in one at a time.  SCRAPPIE_HIP_COALESCE=0 or SCRAPPIE_HIP_BATCH_COALESCE=0: no sharing. */
int scrappie_hip_basecall_batch(scrappie_hip_engine *e, int model,
                                const raw_table *reads, size_t n,
                                const scrappie_hip_params *p, scrappie_hip_call *out);
/* (tests, tools) out[0..2] = engine calls made for shared small calls, caller calls in them, the most callers in one */
void scrappie_hip_batch_coalescer_stats(unsigned long long out[3]);

/* The same on SEVERAL engines (one per GPU of a node; engines[k] holds the model as models[k]).  The
 * reference's parallel axis is reads, `#pragma omp parallel for schedule(dynamic)` (src/scrappie_raw.c:355,387);
 * here reads are sorted by length, cut into launch groups, and each engine's host thread takes the next
 * group from an atomic cursor whenever it has room (two groups in flight per engine).  out[i] <-> reads[i].
 * No data moves between GPUs.  The engines must not be used by other threads meanwhile. */
int scrappie_hip_basecall_batch_multi(scrappie_hip_engine *const *engines, const int *models, size_t nengine,
                                      const raw_table *reads, size_t n, const scrappie_hip_params *p,
                                      scrappie_hip_call *out);
/* The hand-out plan of the call above (host only, no device): order[] takes the read indices sorted by
 * length, longest first; starts[] the first position (in that order) of each launch group; returns the
 * number of groups (even if > cap), -1 if one read alone exceeds max_blocks. */
long scrappie_hip_plan_dynamic(const uint32_t *lengths, size_t n, int stride, size_t nengine, size_t max_reads,
                               size_t max_blocks, uint32_t *order, size_t *starts, size_t cap);
/* Chain-bound reads (host only).  A read is a serial chain of blocks (recurrent layers of alternating direction, decoder, traceback),
 * so a launch group lasts at least as long as its longest read whatever else the device does.  scrappie_hip_basecall_batch
 * therefore runs the reads whose own chain exceeds what the whole call would take with the device full on a helper
 * engine of the same device, beside the launch groups of the others (the GPU analogue of a long read occupying one thread of
 * the reference's schedule(dynamic) loop, src/scrappie_raw.c:355-400).  is_long[n] gets 0 / 1: longest first, at most
 * max_long_blocks column blocks (0: no limit) and 15 % of the call's blocks; returns their number (0: the call is not split).
 * SCRAPPIE_HIP_TAIL=0 in the environment turns the split off. */
long scrappie_hip_plan_tail(const uint32_t *lengths, size_t n, int stride, size_t max_long_blocks, unsigned char *is_long);
/* scrappie_hip_basecall_batch that does not wait for its chain-bound reads.  Their calls are collected later, so the launch groups
 * of the NEXT calls run beside them as well, and the helper engine takes the long reads of all the calls waiting for it as ONE
 * launch group (which lasts as long as its longest read however many it holds): a stream of calls with long-tailed read lengths
 * runs at the device's rate instead of one longest-read chain per call.  deferred[n] gets 1 for the reads whose out[] entry is
 * still blank.  Returns a ticket (> 0) if any read was deferred, 0 if none, -1 on error.  The deferred reads' signals must stay
 * valid until their ticket has been collected.  One host thread per engine.  The helper engine is created by the first call that
 * has chain-bound reads and stays: from then on the engine's launch groups may take 45 % of the device's memory instead of 70 %
 * (the helper 30 % -- SCRAPPIE_HIP_TAIL_MEM, (0 .. 0.4] -- or two helpers, SCRAPPIE_HIP_TAIL=2, 15 % each), i.e. later calls are cut
 * into slightly smaller launch groups. */
long scrappie_hip_basecall_batch_deferred(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n,
                                          const scrappie_hip_params *p, scrappie_hip_call *out, unsigned char *deferred);
/* ... for signals already on the device (scrappie_hip_prep_run): the chain-bound reads are copied back into host memory the ticket
 * owns, so d_signal may be reused as soon as the call returns; tickets are collected as above */
long scrappie_hip_basecall_device_deferred(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets,
                                           const uint32_t *lengths, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out,
                                           unsigned char *deferred);
/* The calls of a ticket's deferred reads, in the order those reads had in their call.  wait = 0: -2 if they are not ready yet.
 * Returns their number; -1 on error (unknown ticket, cap too small, or the helper's launch group failed: the ticket is gone). */
long scrappie_hip_deferred_collect(scrappie_hip_engine *e, long ticket, scrappie_hip_call *out, size_t cap, int wait);

/* Device-resident variant (bench / pipelines that already hold signal in HBM):
 * d_signal is a DEVICE pointer to concatenated normalised samples; read i is
 * d_signal[offsets[i] .. offsets[i]+lengths[i]).  offsets/lengths are host. */
int scrappie_hip_basecall_device(scrappie_hip_engine *e, int model,
                                 const float *d_signal, const uint64_t *offsets,
                                 const uint32_t *lengths, size_t n,
                                 const scrappie_hip_params *p, scrappie_hip_call *out);

/* Signal preparation on the device (k_p0, sh_p0.h): what calculate_post does to a read before the network sees it
 * (src/scrappie_raw.c:270-277) -- trim_and_segment_raw (src/scrappie_common.c:5-73) and medmad_normalise_array
 * (src/util.c:190-205) -- for a whole batch of reads in one launch, bit-identical to the host functions above (windows
 * and samples).  A preparer belongs to one GPU and owns a stream and three slots of buffers (0, 1, 2), so that batch k+1
 * can be prepared (by another host thread) while the engine of the same GPU still reads batch k's signals -- and, with the streaming
 * call below, the last launch group of batch k-1.
 *   scrappie_hip_prep_run: reads[i].raw[0 .. n) are RAW samples (as scrappie_hip_read_raw returns them), reads[i].start /
 *   .end the window at entry.  The samples are gathered into pinned memory, copied to the device, prepared there;
 *   on return *d_signal is the slot's DEVICE buffer, read i's prepared window is d_signal[offsets[i] .. + lengths[i]),
 *   start[i] / end[i] are the window within the read as trim_and_segment_raw would have left rt.start / rt.end;
 *   lengths[i] = 0 where it returns an empty raw_table (nothing left of the read).  offsets / lengths feed
 *   scrappie_hip_basecall_device as they are.  The slot's buffer stays valid until the slot is used again.
 *   varseg_chunk = 0 (a division by zero in the reference) skips trim_raw_by_mad: only the fixed trims apply.
 *   Returns 0, -1 on error (scrappie_hip_last_error). */
typedef struct scrappie_hip_prep scrappie_hip_prep;
scrappie_hip_prep *scrappie_hip_prep_create(int device);
void scrappie_hip_prep_destroy(scrappie_hip_prep *p);
int scrappie_hip_prep_run(scrappie_hip_prep *p, int slot, const raw_table *reads, size_t n,
                          size_t trim_start, size_t trim_end, size_t varseg_chunk, float varseg_thresh,
                          const float **d_signal, uint64_t *offsets, uint32_t *lengths,
                          uint32_t *start, uint32_t *end);
/* The slot's pinned staging buffer handed out piece by piece (thread safe: an atomic cursor): scrappie_hip_prep_begin(slot,
 * capacity in samples) resets the cursor and makes room; scrappie_hip_prep_alloc (a scrappie_hip_sample_alloc; ctx = what
 * _begin returned) gives nsample floats of it, or NULL once the capacity is used up (the reader then mallocs).
 * scrappie_hip_prep_run recognises reads whose .raw lies in the slot's staging buffer and copies only the others.
 * scrappie_hip_prep_owns: whether a pointer lies in the slot's staging buffer (such samples are not the caller's to free). */
void *scrappie_hip_prep_begin(scrappie_hip_prep *p, int slot, size_t capacity_samples);
/* pinned and device buffers of a slot for batches of up to capacity_samples, ahead of time (only while nothing reads the slot;
 * scrappie_hip_prep_begin itself never touches the device side: the engine may still be reading the slot's previous batch) */
int scrappie_hip_prep_reserve(scrappie_hip_prep *p, int slot, size_t capacity_samples);
float *scrappie_hip_prep_alloc(void *ctx, size_t nsample);
int scrappie_hip_prep_owns(scrappie_hip_prep *p, int slot, const float *ptr);
/* copy count prepared samples of the slot, from sample `offset` on, to the host (tests; the CLI never needs them) */
int scrappie_hip_prep_fetch(scrappie_hip_prep *p, int slot, uint64_t offset, size_t count, float *dst);
/* milliseconds the last scrappie_hip_prep_run of the slot spent in (gather on the host, host-to-device copy, k_p0) */
void scrappie_hip_prep_timing(scrappie_hip_prep *p, int slot, double out[3]);

/* Streaming form of scrappie_hip_basecall_device: returns while the call's LAST launch group is still running; that group's calls
 * are delivered -- into the same out[] -- by the next scrappie_hip_basecall_device_stream call on the engine (behind that call's first
 * launch: the engine's two-deep pipeline never drains between batches) or by scrappie_hip_stream_flush; until then those out[] entries
 * are blank (basecall == NULL, score NAN).  out[] and d_signal of a call must stay valid until then.  Any other batched call on the
 * engine delivers the carried group first.  If a call fails, the carried group's calls are lost too (entries stay blank). */
int scrappie_hip_basecall_device_stream(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets,
                                        const uint32_t *lengths, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out);
int scrappie_hip_stream_flush(scrappie_hip_engine *e);
int scrappie_hip_stream_pending(scrappie_hip_engine *e);      /* 1: the last streaming call's last launch group has not been delivered yet */
/* scrappie_hip_basecall_device_deferred whose reads that are not deferred are streamed as above, whether or not the call defers
 * any: out[] entries of the last launch group stay blank until the next streaming call or the flush delivers them; the deferred
 * reads' entries until scrappie_hip_deferred_collect */
long scrappie_hip_basecall_device_deferred_stream(scrappie_hip_engine *e, int model, const float *d_signal, const uint64_t *offsets,
                                                  const uint32_t *lengths, size_t n, const scrappie_hip_params *p, scrappie_hip_call *out,
                                                  unsigned char *deferred);

/* Make the engine's arenas (device and pinned) and code objects ready for launch groups of n reads of `samples` samples: runs one
 * such group on all-zero signals and discards it.  Optional; without it the first calls grow the arenas as they go. */
int scrappie_hip_warm_up(scrappie_hip_engine *e, int model, size_t n, size_t samples);

/* Lower-level, asynchronous: enqueue the device part for reads already in HBM (metadata upload,
 * kernels, D2H of the paths into pinned buffers) and return; scrappie_hip_collect waits for that
 * launch group and stitches it on the host.  The engine holds TWO launch groups, so group k+1 can be
 * enqueued before group k is collected (its kernels then hide the stitching of group k); collect
 * always takes the OLDEST group in flight and its n must match; a third enqueue without a collect is
 * refused.  d_signal must stay valid until the group has been collected.  Returns total blocks, < 0
 * on error.  One thread drives an engine at a time (the per-read functions of the reference surface
 * take the default engine's lock themselves). */
long scrappie_hip_run_device(scrappie_hip_engine *e, int model, const float *d_signal,
                             const uint64_t *offsets, const uint32_t *lengths, size_t n,
                             const scrappie_hip_params *p);
/* wait for the oldest launch group in flight and stitch it on the host (homopolymer correction,
 * k-mer overlap); out[i] describes read i of that group */
int scrappie_hip_collect(scrappie_hip_engine *e, const scrappie_hip_params *p,
                         scrappie_hip_call *out, size_t n);

void scrappie_hip_free_calls(scrappie_hip_call *calls, size_t n);

/* Block-based mapping, batched (sh_eng_map.inc): the network and S1 of a transducer model (a CRF model: see below) run as
 * for scrappie_hip_posterior, the posterior stays on the device, k_map maps every read to its target and only scores
 * and paths return.  reads[i] is mapped to targets[i]; out[i] belongs to reads[i].  seq holds state codes (as
 * encode_bases_to_integers makes them with the model's k-mer length); poslow / poshigh NULL: unbanded, else one entry
 * per block of the read (scrappie_hip_read_blocks).  Parameters: min_prob, tempW, tempb, stay_pen, skip_pen, local_pen
 * of p.  viterbi 0: forward scores.  want_path: the Viterbi path of every unbanded read (malloc'd nblock int32, -1 in
 * START / END); banded reads and forward scores have none.  A read that cannot be mapped (too short, out of the
 * operand range, a bad sequence or band, longer than the limits of DESIGN.md) gets score NAN and path NULL; the others
 * are untouched.  Returns 0, or -1 with scrappie_hip_last_error() when the call as a whole fails.  Takes the engine's
 * call lock, as scrappie_hip_basecall_batch does: calls on one engine run one at a time. */
typedef struct { const int *seq; size_t seqlen; const size_t *poslow, *poshigh; } scrappie_hip_map_target;
typedef struct { float score; size_t nblock; int32_t *path; } scrappie_hip_map_result;
int scrappie_hip_read_blocks(scrappie_hip_engine *e, int model, size_t nsample);   /* posterior columns of a read of nsample samples (0: below the minimum) */
int scrappie_hip_model_states(scrappie_hip_engine *e, int model);                  /* posterior rows (4^k + 1 for a transducer), -1: no such model */
int scrappie_hip_map_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets,
                           size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_result *out);
void scrappie_hip_free_map_results(scrappie_hip_map_result *r, size_t n);
/* the last scrappie_hip_map_batch call's time, milliseconds summed over its launch groups: [0] network + S1, [1] k_map,
 * [2] k_map_walk + results to the host (host clock, the stream drained between the stages) */
void scrappie_hip_map_timing(scrappie_hip_engine *e, double out[3]);
/* states up to which k_map keeps its score rows and the codes in LDS; longer sequences keep the rows in device scratch */
size_t scrappie_hip_map_lds_max_seq(void);

/* One read against many candidate sequences (sh_eng_map_pack.inc; k_map_pack, sh_map_pack.h): which of these barcodes, alleles,
 * edited calls or references is this read?  The network and S1 run ONCE per read; reads[i] is mapped, unbanded, to every
 * cands[i].cand[k], the candidates of a read packed end to end into workgroups of k_map_pack (a candidate too long for a pack
 * takes k_map on the same resident posterior).  out[i].score[k] (malloc'd, ncand floats) belongs to cands[i].cand[k] and is the raw
 * score map_to_sequence_viterbi / _forward give for that pair, bit for bit what scrappie_hip_map_batch gives: candidates of
 * different lengths are compared as they are, and normalising (per block, per base, against a background) is the caller's
 * business.  best: the index of the highest finite score, the lowest index on a tie, -1 where there is none.  With viterbi and
 * want_path, path is the best candidate's Viterbi path (malloc'd nblock int32, -1 in START / END) from a second pass of k_map on
 * that candidate alone while the posterior is still resident -- scrappie_hip_map_batch's path for the pair; NULL otherwise.
 * A candidate that cannot be mapped (no or an empty sequence, a state outside the model's) gets NAN and its neighbours are scored;
 * a candidate with poslow / poshigh set gets NAN too: bands are not part of this call.  A read that cannot run (too short, out of
 * the operand range, over the launch budget) gets every score NAN and best -1, the other reads untouched; the first such reason is
 * the error text.  ncand == 0 is a read with no scores.  Several reads may point at the same cand array (one set of barcodes
 * for all): it is checked, packed and uploaded once.  A CRF model: -1 with a text.  Locks, parameters and
 * the cut into launch groups as scrappie_hip_map_batch; scrappie_hip_map_timing covers these calls ([1] k_map_pack + k_map, [2] walk + results). */
typedef struct { const scrappie_hip_map_target *cand; size_t ncand; } scrappie_hip_map_candidates;
typedef struct { float *score; size_t ncand; int best; size_t nblock; int32_t *path; } scrappie_hip_map_multi_result;
int scrappie_hip_map_multi_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *cands,
                                 size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_multi_result *out);
void scrappie_hip_free_map_multi_results(scrappie_hip_map_multi_result *r, size_t n);
/* per-read surface, process-default engine: a host log-posterior as map_to_sequence_viterbi takes it against ncand candidates,
 * score[k] for cand[k] (NAN where that candidate cannot be mapped or is banded).  0, or -1 with the reason. */
int scrappie_hip_map_post_multi(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen,
                                const scrappie_hip_map_target *cand, size_t ncand, int viterbi, float *score);
/* The packing on the host, no device (sh_host.c): candidates of seqlen[k] states (seqlen[k] + 2 cells: the states, START, END) go
 * into packs of at most pack_cells cells in input order; pack[k] the pack, cell[k] the candidate's first cell in it; pack[k] = -1
 * where the candidate's cells exceed scrappie_hip_map_pack_max_cells() (the cells whose rows and tables fit k_map_pack's LDS) --
 * it takes k_map.  Returns the number of packs.  The debug option "map_pack_cells" sets an engine's pack_cells (0: every candidate
 * through k_map, one workgroup each; -1: the default; a NULL engine: the process-default engine). */
long scrappie_hip_map_pack_plan(const size_t *seqlen, size_t ncand, size_t pack_cells, int *pack, long long *cell);
size_t scrappie_hip_map_pack_max_cells(void);
/* launches of each k_map_pack form in this process, all engines together: index (viterbi ? 2 : 0) | (tiled ? 1 : 0) */
void scrappie_hip_map_pack_form_counts(uint64_t forms[4]);

/* Reads of a flip-flop (CRF) model mapped to base sequences (k_map_crf, sh_map_crf.h; sh_eng_map_crf.inc): decode_crf's recursion
 * (src/decode.c:836-893) restricted to the paths that spell the sequence.  The reference has no such function; the definition is
 * decode_crf's own: a path has nblock + 1 entries, its non-stay entries in order are exactly seq (global: all of the read, all of
 * the sequence, no penalties), float32 as transition + previous, candidates in decode_crf's order (from-state ascending, stay last,
 * replaced on strict >; a base wins a tie at the end).  Mapping a read to its own call returns decode_crf's score bit for bit, and
 * its path.  The forward forms sum over the same paths (logsumexpf, util.h:162-164).
 *
 * scrappie_hip_map_batch with a CRF model: targets[i].seq holds base codes 0..3 and seqlen bases; poslow / poshigh, when given, hold
 * nblock + 1 entries -- one per ENTRY of the path -- and cell index p (the bases emitted so far, 0 .. seqlen) of entry t must lie in
 * [poslow[t], poshigh[t]) (scrappie_hip_map_crf_bounds_sane); out[i].nblock is the read's block count and out[i].path, for every
 * read of a Viterbi call with want_path, banded or not, has nblock + 1 entries: path[t] = index of the last base emitted through
 * entry t, -1 while none (entry t is a base exactly where path[t] > path[t - 1]).  stay_pen, skip_pen and local_pen are not used.
 * A sequence with no admissible path (seqlen > nblock + 1, or a band that excludes them all: a score below -1e30 / 2) gets NAN and
 * an error text, as every other read that cannot be mapped.  Launch groups are cut by the same cost model (a CRF model's posterior
 * is its 25 transitions per block), k_map_crf runs on the transitions where k_crf left them, and scrappie_hip_map_timing covers
 * these calls ([1] k_map_crf, [2] k_map_crf_walk + results).  Transducer models go through exactly what they went through before.
 *
 * The per-read symbols run on the process-default engine: trans as nanonet_rnnrf_r94_transitions returns it (25 rows, element
 * to * 5 + from, states A C G T stay; nc >= 1 blocks), uploaded, one launch.  path: nblock + 1 entries, may be NULL.  low / high:
 * nblock + 1 entries each.  NAN with scrappie_hip_last_error() on a null argument, a matrix that is not 25 rows with at least one
 * block, a base code outside 0..3, a sequence longer than the limit of DESIGN.md, an invalid band, or no admissible path. */
float map_crf_to_sequence_viterbi(const_scrappie_matrix trans, int const *seq, size_t seqlen, int *path);
float map_crf_to_sequence_forward(const_scrappie_matrix trans, int const *seq, size_t seqlen);
float map_crf_to_sequence_viterbi_banded(const_scrappie_matrix trans, int const *seq, size_t seqlen, size_t const *low, size_t const *high, int *path);
float map_crf_to_sequence_forward_banded(const_scrappie_matrix trans, int const *seq, size_t seqlen, size_t const *low, size_t const *high);
/* Host only.  A band is valid when low[0] == 0, high[nblock] == seqlen + 1, low[t] < high[t] <= seqlen + 1, both are non-decreasing
 * and low[t] <= high[t - 1] (t = 0 .. nblock): 1, else 0 (quiet). */
int scrappie_hip_map_crf_bounds_sane(const size_t *low, const size_t *high, size_t nblock, size_t seqlen);
/* Host only.  The diagonal through (entry 0, cell 0) and (entry nblock, cell seqlen), halfwidth cells to either side, clamped so that
 * the result is always valid; low and high take nblock + 1 entries each.  0, or -1 on a null or empty argument. */
int scrappie_hip_map_crf_diagonal_band(size_t nblock, size_t seqlen, size_t halfwidth, size_t *low, size_t *high);
/* bases up to which k_map_crf keeps its score rows and the codes in LDS; longer sequences keep the rows in device scratch */
size_t scrappie_hip_map_crf_lds_max_seq(void);
/* The planner's scratch arithmetic on the host, no device (for the tests): as scrappie_hip_map_plan_scratch; k_map_crf touches
 * 4 (seqlen + 2) floats from its offset. */
long long scrappie_hip_map_crf_plan_scratch(const size_t *seqlen, const size_t *nblock, size_t n, long long *off);
/* launches of each k_map_crf form in this process, all engines together: index (viterbi ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
void scrappie_hip_map_crf_form_counts(uint64_t forms[8]);

/* One read of a flip-flop (CRF) model against many candidate sequences (sh_eng_map_crf_pack.inc; k_map_crf_pack, sh_map_crf_pack.h): which of
 * these alleles, haplotypes or references is this read, is this edit of the call better than the call?  scrappie_hip_map_multi_batch's
 * question for the model whose score is a proper path score.  The network and k_crf run ONCE per read; reads[i] is mapped, unbanded, to every
 * cands[i].cand[k] (base codes 0..3), the candidates of a read packed end to end into workgroups of k_map_crf_pack on the transitions where
 * k_crf left them (a candidate of more than scrappie_hip_map_crf_pack_max_cells() - 1 bases takes k_map_crf on the same transitions).
 * out[i].score[k] (malloc'd, ncand floats; freed by scrappie_hip_free_map_multi_results) is the score map_crf_to_sequence_viterbi / _forward
 * give for that pair, bit for bit what scrappie_hip_map_batch gives.  best: the index of the highest finite score, the lowest index on a tie,
 * -1 where there is none.  With viterbi and want_path, path is the best candidate's Viterbi path (malloc'd, nblock + 1 int32, as
 * scrappie_hip_map_batch gives for that pair) from a second pass of k_map_crf on that candidate alone while the transitions are still resident;
 * NULL otherwise.  stay_pen, skip_pen and local_pen are not used.  A candidate gets NAN, and its neighbours are scored, where it has no or an
 * empty sequence, a code that is not a base, poslow / poshigh set ("bands are not part of this call"), or no admissible path (seqlen >
 * nblock + 1: a score below -1e30 / 2); the first such reason is the error text.  A read that cannot run (too short, out of the operand range,
 * over the launch budget) gets every score NAN and best -1, the other reads untouched.  ncand == 0 is a read with no scores.  Several reads
 * may point at the same cand array: it is checked, packed and uploaded once.  A transducer model: -1 with a text that names
 * scrappie_hip_map_multi_batch.  Locks, parameters and the cut into launch groups as scrappie_hip_map_batch with a CRF model, a read adding its
 * candidates' tables and, with a path, the second pass on its longest candidate; scrappie_hip_map_timing covers these calls
 * ([1] k_map_crf_pack + k_map_crf, [2] walk + results). */
int scrappie_hip_map_crf_multi_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *cands,
                                     size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_multi_result *out);
/* per-read surface, process-default engine: a host matrix as map_crf_to_sequence_viterbi takes it against ncand candidates, score[k] for cand[k]
 * (NAN where that candidate cannot be mapped, is banded or has no admissible path; the first reason is the error text).  0, or -1 with the reason. */
int scrappie_hip_map_trans_multi(const_scrappie_matrix trans, const scrappie_hip_map_target *cand, size_t ncand, int viterbi, float *score);
/* The packing on the host, no device (sh_host.c): candidates of seqlen[k] bases (seqlen[k] + 1 cells: p = 0 .. seqlen bases emitted) go into
 * packs of at most pack_cells cells in input order; pack[k] the pack, cell[k] the candidate's first cell in it; pack[k] = -1 where the
 * candidate's cells exceed scrappie_hip_map_crf_pack_max_cells() (what k_map_crf_pack's LDS holds: 64 + 5 (cells + 1) words within 64 KB) --
 * it takes k_map_crf and closes no pack.  Returns the number of packs.  The debug option "map_crf_pack_cells" sets an engine's pack_cells
 * (0: every candidate through k_map_crf, one workgroup each; -1: the default; a NULL engine: the process-default engine). */
long scrappie_hip_map_crf_pack_plan(const size_t *seqlen, size_t ncand, size_t pack_cells, int *pack, long long *cell);
size_t scrappie_hip_map_crf_pack_max_cells(void);
/* launches of each k_map_crf_pack form in this process, all engines together: index (viterbi ? 2 : 0) | (tiled ? 1 : 0) */
void scrappie_hip_map_crf_pack_form_counts(uint64_t forms[4]);

/* Reads of a flip-flop (CRF) model mapped INTO a longer sequence (k_map_crf_local, sh_map_crf_local.h; sh_eng_map_crf_local.inc): where
 * in this sequence does the read lie, with what score and along what path.  Cells, transitions and the block recursion are those
 * above; the path may begin in any cell (entry 0: S[p] = 0 for p = 0 .. seqlen, B[p] = 0 for p = 1 .. seqlen, as decode_crf starts
 * every state at 0) and end in any cell (Viterbi: the maximum over all cells of entry nblock, p ascending and B[p] before S[p], the
 * first maximum wins; forward: logsumexpf over them).  The read spells seq[first, last): last is the end cell's p, first the start
 * cell's p, minus one where entry 0 is a base; path[t], t = 0 .. nblock, is the index in seq of the last base emitted through
 * entry t, first - 1 while there is none.  The all-stay path is always admissible: there is no "no path" here.  Mapping a read to
 * flank + its own call (the bases of all nblock + 1 entries) + flank returns decode_crf's score bit for bit, and never less than
 * map_crf_to_sequence_viterbi gives for the same pair.
 * The sequence is cut into windows of one workgroup each (scrappie_hip_map_crf_local_plan); the Viterbi score has the same bits for
 * every cut.  seqlen has no limit from the device's LDS; it is bounded by index width alone: 2^30 bases.
 *
 * scrappie_hip_map_local_batch: reads[i] (prepared as for scrappie_hip_map_batch) into targets[i] = {seq, seqlen}, base codes 0..3;
 * several reads may point at the same seq (with the same seqlen), which is then checked and uploaded once per launch group.  A
 * first pass scores every window of every read of a launch group in one launch; with viterbi and want_path a second launch runs the
 * traceback on each read's best window alone, while the transitions are still resident.  out[i]: score (NAN where read or sequence
 * cannot be mapped, with the first such reason as the error text; its neighbours are untouched), nblock, last (Viterbi; 0 for
 * forward), first (known from the traceback only: (size_t)-1 without viterbi and want_path), path (nblock + 1 entries, malloc'd;
 * scrappie_hip_free_map_local_results).  A transducer model is refused for the
 * whole call (-1).  scrappie_hip_map_timing covers the call ([1] k_map_crf_local, [2] walk + results).
 *
 * The per-read symbols run on the process-default engine; NULL / NAN conventions as map_crf_to_sequence_*; first, last and path may
 * each be NULL, and a call that wants neither first nor path runs the first pass alone. */
typedef struct { const int *seq; size_t seqlen; } scrappie_hip_map_local_target;
typedef struct { float score; size_t nblock, first, last; int32_t *path; } scrappie_hip_map_local_result;
int scrappie_hip_map_local_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_local_target *targets,
                                 size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_local_result *out);
void scrappie_hip_free_map_local_results(scrappie_hip_map_local_result *r, size_t n);
float map_crf_to_reference_viterbi(const_scrappie_matrix trans, int const *seq, size_t seqlen, size_t *first, size_t *last, int *path);
float map_crf_to_reference_forward(const_scrappie_matrix trans, int const *seq, size_t seqlen);
/* Host only: the cut of seqlen + 1 cells into windows for a read of nblock blocks.  stride > 0: cells per window's owned starts; 0:
 * one window; < 0: the default (the debug option "map_crf_local_stride" takes the same values) -- a window of stride + nblock =
 * 2034 cells (four such workgroups are resident per compute unit) while that leaves stride >= nblock; beyond, the largest stride
 * whose window keeps its rows in LDS (scrappie_hip_map_crf_local_max_cells); and nblock, rows in device scratch, where nblock + 1
 * cells alone exceed that.  Window w owns the start cells [first[w], first[w] + own[w]) and holds ncell[w] cells from
 * first[w]; home[w]: 0 LDS, 1 scratch at float offset scr_off[w] (-1 in LDS; 4 (ncell + 1) floats each) of *scr_floats in all.  Arrays
 * may be NULL and hold cap entries.  Returns the number of windows; 0 where there is nothing to cut or seqlen exceeds 2^30. */
long long scrappie_hip_map_crf_local_plan(size_t seqlen, size_t nblock, long stride, size_t cap, size_t *first, size_t *ncell, size_t *own,
                                          int *home, long long *scr_off, long long *scr_floats);
size_t scrappie_hip_map_crf_local_stride(size_t seqlen, size_t nblock, long stride);
size_t scrappie_hip_map_crf_local_max_cells(void);
/* launches of each k_map_crf_local form in this process, all engines together: index (viterbi ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
void scrappie_hip_map_crf_local_form_counts(uint64_t forms[8]);

/* Reads of a transducer model mapped INTO a longer sequence of k-mer states (k_map_local, sh_map_local.h; sh_eng_map_local.inc): where
 * in this amplicon, plasmid or chromosome arm does the read lie.  It is map_to_sequence_viterbi / _forward (decode.c:1420-1640,
 * unbanded) with the sequence side made local: the states are the positions 0 .. seqlen - 1, START, and one END accumulator per
 * position; START = 0 before block 0 and everything else -1e30.  Per block, from the previous row p to c, lps the stay entry, le
 * the entry of state seq[pos], ls = fmaxf(-local_pen, lps):
 *   c[START] = p[START] + ls
 *   c[pos] = (p[pos] - stay_pen) + lps, then on strict > in this order step p[pos - 1] + le (pos >= 1), skip (p[pos - 2] -
 *            skip_pen) + le (pos >= 2), from START p[START] + le for every pos (the reference: at pos 0 only)
 *   E'[pos] = E[pos] + ls, then p[pos] - local_pen on strict > (any position may leave for END; the reference: seqlen - 1 only)
 * After the last block x is the first maximum of c[pos] and y the first maximum of E[pos], pos ascending; the score is
 * fmaxf(x, y) and the path ends in a sequence cell iff x > y; START is no end state.  Forward: logsumexpf in place of every max.
 * path[blk], nblock entries: the position in seq, -1 in START / END; first: the lowest position the path visits, last: the highest
 * plus one -- with a k-mer model the read spells bases first .. last + k - 2 of the base string.  A path always exists, and the
 * score is never below map_to_sequence_viterbi's for the same pair.
 * The sequence is cut into windows of one workgroup each (scrappie_hip_map_local_plan); the Viterbi score has the same bits for
 * every cut.  seqlen is bounded by index width alone: 2^30 states; the posterior by what a workgroup stages: 2048 states.
 *
 * scrappie_hip_map_post_local_batch: reads[i] (prepared as for scrappie_hip_map_batch) into targets[i] = {seq, seqlen}, state codes
 * as encode_bases_to_integers gives them; several reads may point at the same seq (with the same seqlen), which is then checked
 * and uploaded once per launch group.  p: min_prob, tempW, tempb and the three penalties.  Two passes as
 * scrappie_hip_map_local_batch; out[i]: score (NAN where read or sequence cannot be mapped, with the first such reason as the error
 * text; its neighbours are untouched), nblock, last (Viterbi; 0 for forward), first (known from the traceback only: (size_t)-1
 * without viterbi and want_path), path (nblock entries, malloc'd; scrappie_hip_free_map_local_results).  A flip-flop (CRF) model is
 * refused for the whole call (-1): its call is scrappie_hip_map_local_batch.  scrappie_hip_map_timing covers the call.
 *
 * The per-read symbols run on the process-default engine on a posterior of log-probabilities as map_to_sequence_* take it, whose
 * columns are whole 16-byte pieces apart (scrappie matrices are); first, last and path may each be NULL, and a call that wants
 * neither first nor path runs the first pass alone. */
float map_to_reference_viterbi(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen, int const *seq, size_t seqlen,
                               size_t *first, size_t *last, int *path);
float map_to_reference_forward(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen, int const *seq, size_t seqlen);
int scrappie_hip_map_post_local_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_local_target *targets,
                                      size_t n, const scrappie_hip_params *p, int viterbi, int want_path, scrappie_hip_map_local_result *out);
/* Host only: the cut of seqlen positions into windows for a read of nblock blocks of a posterior of nr states.  A path advances at
 * most reach = 2 (nblock - 1) positions.  stride > 0: entry positions per window; 0: one window; < 0: the default (the debug option
 * "map_local_stride" takes the same values) -- while a window with stride > reach keeps its rows in LDS
 * (scrappie_hip_map_local_max_cells(nr)): a window of stride + reach = 2798 cells (three such workgroups are resident per compute
 * unit) where that leaves a stride of 1200 or more, the largest LDS-resident window for longer reads; and 2 nblock, rows in
 * device scratch, beyond that.  Window w owns the entry positions [first[w], first[w] + own[w]) and holds ncell[w] cells from
 * first[w]; home[w]: 0 LDS, 1 scratch at float offset scr_off[w] (-1 in LDS; 3 * 4 ceil(ncell / 4) floats each) of *scr_floats in
 * all.  Arrays may be NULL and hold cap entries.  Returns the number of windows; 0 where there is nothing to cut. */
long long scrappie_hip_map_local_plan(size_t seqlen, size_t nblock, size_t nr, long stride, size_t cap, size_t *first, size_t *ncell, size_t *own,
                                      int *home, long long *scr_off, long long *scr_floats);
size_t scrappie_hip_map_local_stride(size_t seqlen, size_t nblock, size_t nr, long stride);
size_t scrappie_hip_map_local_max_cells(size_t nr);
/* launches of each k_map_local form in this process, all engines together: index (viterbi ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0) */
void scrappie_hip_map_local_form_counts(uint64_t forms[8]);

/* Short sequences searched INSIDE reads of a flip-flop (CRF) model (k_crf_find, sh_crf_find.h; sh_eng_crf_find.inc): does this
 * barcode, adapter, primer or marker occur somewhere in the read, where, and which of K such motifs fits best.  Viterbi only.  A
 * path (nblock + 1 entries over A C G T stay, as decode_crf's) is admissible for a motif m[0..L) when it has entries begin <= end,
 * both bases, such that the non-stay entries in [begin, end] are exactly m in order; the entries before begin and behind end are
 * free.  The score is decode_crf's sum over the best such path, so it covers the whole read: scores of motifs of different
 * lengths compare as they are, and score - call_score <= 0 is a log-odds against the read's own call (call_score: decode_crf's
 * score, bit for bit).  score == call_score in bits where the motif is a run of consecutive bases of the read's call, and score is
 * never below map_crf_to_sequence_viterbi's for the same pair.  begin and end are entries of the path, 0 .. nblock (entry t lies
 * between blocks t - 1 and t: sample t * stride of the trimmed signal).  There is no forward form: a path whose call holds the
 * motif twice has several decompositions, and a sum would count it more than once.
 * The motifs of a read are packed end to end into workgroups (scrappie_hip_crf_find_plan) behind the read's own five cells; a
 * motif's score does not depend on its neighbours or on the pack size.
 *
 * scrappie_hip_find_batch: reads[i] (prepared as for scrappie_hip_map_batch) against motifs[i] = {cand, ncand}, base codes 0..3 in
 * cand[k].seq; several reads may point at the same cand array, which is then checked, packed and uploaded once per launch.  out[i]:
 * score, begin, end (malloc'd, nmotif entries each; begin and end NULL without want_pos; NAN and -1 where a motif cannot be
 * searched: empty, not bases, banded (poslow / poshigh set), "too long for k_crf_find" -- more than
 * scrappie_hip_crf_find_max_cells() - 9 bases; long sequences are map_to_sequence's and map_to_reference's job -- or longer than the
 * read's nblock + 1 entries; its neighbours are scored), call_score, best (the highest finite score, the lowest index on a tie,
 * -1: none) and nblock.  A read that cannot run (too short, out of the operand range, over the launch budget) gets every score NAN
 * and best -1, the other reads untouched; the first such reason is the error text.  A transducer model: -1 with a text that
 * names it.  Locks, parameters and the cut into launch groups as scrappie_hip_map_batch; all packs of all reads of a launch group
 * go in one launch; scrappie_hip_map_timing covers the call ([1] k_crf_find, [2] results).
 *
 * find_crf_sequences_viterbi: the same on a host matrix (as nanonet_rnnrf_r94_transitions returns it) and the process-default
 * engine; score[k] for motif[k], begin and end may be NULL (then positions are not carried), call_score may be NULL.  0, or -1
 * with the reason; 0 with an error text where some motif got NAN. */
typedef struct { float *score; int32_t *begin, *end; size_t nmotif; float call_score; int best; size_t nblock; } scrappie_hip_find_result;
int scrappie_hip_find_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_candidates *motifs, size_t n,
                            const scrappie_hip_params *p, int want_pos, scrappie_hip_find_result *out);
void scrappie_hip_free_find_results(scrappie_hip_find_result *r, size_t n);
int find_crf_sequences_viterbi(const_scrappie_matrix trans, const scrappie_hip_map_target *motif, size_t nmotif, float *score, int32_t *begin,
                               int32_t *end, float *call_score);
/* Host only: motifs of seqlen[k] bases into packs of at most pack_cells cells (the debug option "crf_find_cells" sets it for an
 * engine, -1: the default of 512; never more than scrappie_hip_crf_find_max_cells(), what the LDS holds), in input order.  A pack
 * begins with the read's five cells, a motif of L bases takes L + 4 behind them; a pack is closed when the next motif would take it
 * past pack_cells.  pack[k], cell[k]: the motif's pack and its first cell there; -1 for an empty motif and one whose L + 9 cells
 * exceed the maximum.  Returns the number of packs. */
long scrappie_hip_crf_find_plan(const size_t *seqlen, size_t nmotif, size_t pack_cells, int *pack, long long *cell);
size_t scrappie_hip_crf_find_max_cells(void);
/* launches of each k_crf_find form in this process, all engines together: index (positions ? 2 : 0) | (tiled ? 1 : 0) */
void scrappie_hip_crf_find_form_counts(uint64_t forms[4]);

/* Every single-base edit of a sequence scored against a read of a flip-flop (CRF) model in one pass (sh_eng_crf_edits.inc;
 * k_crf_edits_rows, k_crf_edits, sh_crf_edits.h): for seq[0..L) the 4 L substitutions (the L that change nothing among them), the L
 * deletions and the 4 (L + 1) insertions, each the score map_crf_to_sequence_viterbi / _forward give for the edited sequence --
 * from one forward sweep, one backward sweep and one combining pass instead of 9 L + 4 dynamic programmes.
 *
 * Definition (tests/test_crf_edits_cpu.py restates it in numpy).  trans[nblock][25], element to * 5 + from, states A C G T stay;
 * NB = nblock, entries t = 0 .. NB, block t leads from entry t to entry t + 1; BIG = 1e30; mx(a, b): b if b > a else a (Viterbi),
 * log(e^a + e^b) (forward), the arguments in the order written.
 *   Forward rows, k_map_crf's cells kept for every entry: F_B[0][1] = F_S[0][0] = 0, everything else -BIG; with b = seq[p - 1]
 *     F_B[t + 1][p] = mx(tr_t[5 b + seq[p - 2]] + F_B[t][p - 1], tr_t[5 b + 4] + F_S[t][p - 1])     (p == 1: the second term alone)
 *     F_S[t + 1][p] = mx(tr_t[20 + b] + F_B[t][p], tr_t[24] + F_S[t][p])                           (p == 0: the second term alone)
 *   base: F_B[NB][L] if it is >= F_S[NB][L], else F_S[NB][L] (Viterbi); their mx (forward): map_crf_to_sequence_*'s score, bit for bit.
 *   Backward rows: G_B[NB][L] = G_S[NB][L] = 0, everything else, column L + 1 throughout, -BIG; for t descending
 *     G_B[t][p] = mx(tr_t[5 seq[p] + seq[p - 1]] + G_B[t + 1][p + 1], tr_t[20 + seq[p - 1]] + G_S[t + 1][p])      (1 <= p)
 *     G_S[t][p] = mx(tr_t[5 seq[p] + 4] + G_B[t + 1][p + 1], tr_t[24] + G_S[t + 1][p])              (p == L: the second terms alone)
 *   An edit is the prefix seq[:i], perhaps a new base c, the suffix seq[j:]: a substitution at i < L (j = i + 1, sub[i][c]), a
 *   deletion at i < L (j = i + 1, no new base, del[i]; NAN where L == 1), an insertion before i <= L (j = i, ins[i][c]).  pb = seq[i - 1]
 *   (none: i == 0), n = seq[j] (none: j == L).  "Enter x after y from (PB, PS) at block t": mx(tr_t[5 x + y] + PB, tr_t[5 x + 4] + PS),
 *   the second term alone where there is no y.
 *     1. the source columns are (F_B[.][i], F_S[.][i]), F_B[.][0] = -BIG;
 *     2. with a new base: X_B[0] = 0 if i == 0, else -BIG; X_S[0] = -BIG; X_B[t + 1] = enter c after pb from the source at t;
 *        X_S[t + 1] = mx(tr_t[20 + c] + X_B[t], tr_t[24] + X_S[t]); X becomes the source and pb = c;
 *     3. no n: the score is base's end rule on the source at NB;
 *     4. else Y[0] = 0 iff nothing precedes n (a deletion at i == 0), else -BIG; Y[t] = enter n after pb from the source at t - 1;
 *        the score is mx over t = 0 .. NB ascending of Y[t] + G_B[t][j + 1], accumulated left to right.
 *   A score below -BIG / 2 is NAN: the edited sequence has more bases than the read has entries.  sub[i][seq[i]] is computed as any other.
 * The join is exact: every path that spells the edited sequence is in the cell of n exactly once.  An edit's score and base are
 * different chains of float32 additions: Viterbi scores of an edit and of map_crf_to_sequence_viterbi on the edited sequence agree to
 * rounding, not in bits; a caller confirms the edits it chooses with scrappie_hip_map_crf_multi_batch, which is exact.
 *
 * scrappie_hip_map_crf_edits_batch: reads[i] (prepared as for scrappie_hip_map_batch) against targets[i] (base codes 0..3, unbanded).
 * out[i]: base, sub (4 seqlen floats, [i][c]), del (seqlen), ins (4 (seqlen + 1), [i][c]), malloc'd, freed by
 * scrappie_hip_free_edits_results; seqlen and nblock.  It runs as scrappie_hip_map_batch does for a CRF model: the network and k_crf
 * once per launch group, then k_crf_edits_rows forward, k_crf_edits_rows backward and k_crf_edits on the main stream while the
 * transitions are resident.  A read adds its three row matrices (scrappie_hip_crf_edits_row_bytes) and its results to the cut
 * into launch groups; the debug option "crf_edits_budget_kb" bounds the row and result bytes of one launch of the three kernels
 * (0: one launch per launch group).  A target that cannot be scored -- no or an empty sequence, a code that is not a base, poslow /
 * poshigh set ("bands are not part of this call"), more than scrappie_hip_map_crf_lds_max_seq() bases ("too long for k_crf_edits":
 * polishing works on windows) -- gets base and every edit NAN and the first such reason is the error text; its neighbours are
 * scored.  A NAN edit is a result, not an error.  A transducer model: -1 with a text that names it.  viterbi 0: forward scores.
 * scrappie_hip_map_timing covers the call ([0] network + k_crf; [1] the three launches with their copies: uploads of records and codes,
 * the kernels, results to the host and the NAN pass over them, by the host's clock; [2] stays 0); scrappie_hip_crf_edits_timing has the
 * kernels alone.
 *
 * map_crf_edits: the same on a host matrix (as nanonet_rnnrf_r94_transitions returns it) and the process-default engine, a batch
 * of one; base, sub, del, ins may each be NULL; all are NAN, the return value 0 and the reason the error text where the sequence cannot
 * be scored.  -1 with the reason: a null argument, not a transition matrix, a failed launch. */
typedef struct { float base; float *sub, *del, *ins; size_t seqlen, nblock; } scrappie_hip_edits_result;
int scrappie_hip_map_crf_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                     const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out);
void scrappie_hip_free_edits_results(scrappie_hip_edits_result *r, size_t n);
int map_crf_edits(const_scrappie_matrix trans, const int *seq, size_t seqlen, int viterbi, float *base, float *sub, float *del, float *ins);
/* Host only (sh_host.c): what a launch of the three kernels keeps on the device.  pitch: floats from one entry's row to the next
 * (seqlen + 2 rounded up to 16); row_bytes: the three row matrices of nblock + 1 entries; plan: reads in input order, rows[i] the
 * float offset of read i's F_B in the row buffer (F_S (nblock[i] + 1) * pitch[i] floats behind it, G_B as many behind F_S), res[i]
 * that of its results (sub [L][4], ins [L + 1][4], del [L]) in the result buffer, both multiples of 4; returns the floats of the row
 * buffer, *res_floats (may be NULL) those of the result buffer. */
size_t scrappie_hip_crf_edits_pitch(size_t seqlen);
size_t scrappie_hip_crf_edits_row_bytes(size_t seqlen, size_t nblock);
long long scrappie_hip_crf_edits_plan(const size_t *seqlen, const size_t *nblock, size_t n, int *pitch, long long *rows, long long *res,
                                      long long *res_floats);
/* launches of each form in this process, all engines together: k_crf_edits_rows at (viterbi ? 4 : 0) | (tiled ? 2 : 0) | (backward ? 1 : 0),
 * k_crf_edits at 8 + ((viterbi ? 2 : 0) | (tiled ? 1 : 0)) */
void scrappie_hip_crf_edits_form_counts(uint64_t forms[12]);
/* the last scrappie_hip_map_crf_edits_batch call on this engine: ms[0..2] the device time of k_crf_edits_rows forward, backward and
 * k_crf_edits (events on the main stream), summed over its launches; *launches (may be NULL): how many launches of the three it made;
 * *row_bytes (may be NULL): the row bytes of all of them */
void scrappie_hip_crf_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes);

/* The same in a band (the kernels' banded forms, sh_crf_edits.h): a read that covers a window lies on a narrow diagonal of the lattice,
 * and rows, traffic and sums are proportional to the cells visited.
 *
 * Definition (tests/test_crf_edits_band_cpu.py restates it in numpy).  A band is what scrappie_hip_map_batch takes for a CRF model: low,
 * high of nblock + 1 entries, cell p (bases emitted so far, 0 .. L) of entry t admissible iff low[t] <= p < high[t]; it must pass
 * scrappie_hip_map_crf_bounds_sane.  The definition above holds with these changes and no other:
 *   F_B, F_S, G_B and G_S hold -BIG at every cell outside the band of its entry: F_B[0][1] = 0 only where high[0] > 1, a cell inside the
 *   band is computed by the recursion from the masked row of the entry before (behind), a cell outside is -BIG.  Column L + 1 of G stays
 *   -BIG throughout.  The recursions, the candidate order, mx, the end rule and the NAN rule are unchanged.
 *   The new base's own cells X_B, X_S carry NO band: a band is given in the coordinates of the original sequence and the new cell has
 *   none there.  sub[i][c] and ins[i][c] go on sharing X.
 * Consequences:
 *   Equivalence.  An edit's score is the score of the banded dynamic programme on the edited sequence in which every cell inherited from
 *     the original -- the prefix's cells 0 .. i keep their index, the suffix's cells their index in the original -- keeps its original
 *     cell's band and the new base's cell (i + 1 of the edited sequence) is free at every entry.
 *   base is map_crf_to_sequence_viterbi_banded / _forward_banded's score for the same band, bit for bit.
 *   Full band.  With low[t] = 0 and high[t] = L + 1 at every entry every output equals map_crf_edits' bit for bit, Viterbi and forward:
 *     the banded forms run through the same cell code (sh_map_crf_cell, sh_ce_mx, sh_ce_end) in the same order.
 *   Identity substitution.  sub[i][seq[i]] is computed as any other substitution: its cell i + 1 is the new base's and free, so it may
 *     EXCEED base where the band binds on cell i + 1.
 *   Ends.  A tight band can make an edit at either end NAN -- del[L - 1] where low[nblock] == L: the deletion closes on cell L - 1 of
 *     entry nblock.  That is a result, not an error; the caller chooses the half-width.
 * Rows on the device: an entry's row holds its band's cells alone, cell p of entry t at float p - low[t], in rows of one pitch per read:
 * the widest entry's cells and one slot for the stores of threads without a cell, rounded up to 16 floats
 * (scrappie_hip_crf_edits_band_pitch); three matrices of nblock + 1 such rows (scrappie_hip_crf_edits_band_row_bytes).  The score rows of
 * k_crf_edits_rows stay in LDS by k_map_crf's formula, so the limit stays scrappie_hip_map_crf_lds_max_seq() bases.  k_crf_edits walks,
 * per workgroup of 256 positions, only the entries at which one of its positions can be alive.
 *
 * scrappie_hip_map_crf_edits_banded_batch: as scrappie_hip_map_crf_edits_batch (same results, same free function, the network once per
 * launch group, three launches); targets[i].poslow / poshigh hold nblock + 1 entries each for the read's nblock, or are both NULL: the
 * full band, run through the unbanded forms.  A read's cost in the cut into launch groups and under "crf_edits_budget_kb" is its banded
 * row bytes.  A band that is not valid for the read's block count (an array made for another block count is not) gets NAN for that read
 * and the first reason as the error text; its neighbours are scored.  A transducer model: -1.  scrappie_hip_crf_edits_timing covers the
 * call, row_bytes the bytes the launches kept.  scrappie_hip_map_crf_edits_batch itself goes on refusing bands.
 * map_crf_edits_banded: a batch of one on a host matrix and the process-default engine, as map_crf_edits; low and high are required. */
int scrappie_hip_map_crf_edits_banded_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                            const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out);
int map_crf_edits_banded(const_scrappie_matrix trans, const int *seq, size_t seqlen, const size_t *low, const size_t *high, int viterbi, float *base,
                         float *sub, float *del, float *ins);
/* Host only.  The band of half-width `halfwidth` cells around a Viterbi path of k_map_crf (path[t], t = 0 .. nblock: the index of the last
 * base emitted through entry t, -1 while none): with cnt = path[t] + 1, low[t] = max(cnt - halfwidth, 0) -- and low[0] = 0 whatever the
 * half-width, as every band begins -- and high[t] = min(cnt + halfwidth + 1, seqlen + 1); nblock + 1 entries each.  The result always
 * passes scrappie_hip_map_crf_bounds_sane and contains the path.  0, or -1 on a null or empty argument or what is no path of that
 * sequence: a value outside -1 .. seqlen - 1 (at entry 0: outside -1 .. 0), a step down, a step above 1, path[nblock] != seqlen - 1. */
int scrappie_hip_map_crf_path_band(const int *path, size_t nblock, size_t seqlen, size_t halfwidth, size_t *low, size_t *high);
/* Host only (sh_host.c), as scrappie_hip_crf_edits_pitch / _row_bytes / _plan for reads in bands: pitch, the floats of an entry's row
 * (0: a null argument); row_bytes, the three matrices; plan, with low[i] / high[i] read i's band of nblock[i] + 1 entries (either NULL:
 * the read has none and takes the unbanded pitch). */
size_t scrappie_hip_crf_edits_band_pitch(const size_t *low, const size_t *high, size_t nblock);
size_t scrappie_hip_crf_edits_band_row_bytes(const size_t *low, const size_t *high, size_t nblock);
long long scrappie_hip_crf_edits_band_plan(const size_t *seqlen, const size_t *nblock, const size_t *const *low, const size_t *const *high, size_t n,
                                           int *pitch, long long *rows, long long *res, long long *res_floats);
/* launches of each banded form in this process, indexed as scrappie_hip_crf_edits_form_counts, which counts the unbanded forms alone */
void scrappie_hip_crf_edits_band_form_counts(uint64_t forms[12]);
/* private (scratch) bytes per lane of each banded form, as the runtime reports them for the loaded kernels, indexed as the form counts (needs
 * a device; -1: the runtime gave no answer).  The forms are built to need none. */
void scrappie_hip_crf_edits_band_scratch(long long bytes[12]);

/* Every single-base edit of a sequence scored against a read of a TRANSDUCER model in one pass (sh_eng_map_edits.inc; k_map_edits_rows,
 * k_map_edits, sh_map_edits.h): for the bases seq[0..L) the 4 L substitutions, the L deletions and the 4 (L + 1) insertions, numbered as
 * above, each the score map_to_sequence_viterbi / _forward give for the k-mer states of the edited sequence -- from one forward sweep,
 * one backward sweep and one combining pass instead of 9 L + 4 dynamic programmes.
 *
 * Definition (tests/test_map_edits_cpu.py restates it in numpy).  lp[t][s]: the read's log-posterior, NB blocks, nr = 4^k + 1 rows, the
 * stay row the last; lps = lp[t][nr - 1]; penalties stay_pen, skip_pen, local_pen; BIG = 1e30; mx(a, b): b if b > a else a (Viterbi),
 * log(e^a + e^b) (forward), the arguments in the order written; ls = mx(-local_pen, lps).  s[q] = kmer(seq[q .. q + k)), q = 0 .. n - 1,
 * n = L - k + 1, the first base the most significant.  Entries t = 0 .. NB; block t leads from entry t to entry t + 1.
 *   The cell rule at index q with state x, reading columns q, q - 1, q - 2 of entry t: (col[t][q] - stay_pen) + lps, then mx with the step
 *     col[t][q - 1] + lp[t][x] (q >= 1), with the skip (col[t][q - 2] - skip_pen) + lp[t][x] (q >= 2), with FS[t] + lp[t][x] from START (q == 0).
 *   Forward rows, map_to_sequence's cells kept for every entry: F[0][q] = -BIG; FS[0] = 0, FS[t + 1] = FS[t] + ls; F[t + 1][q] the cell rule
 *     with state s[q].  base: map_to_sequence_*'s end rule on row NB with its END cell, bit for bit its score.
 *   Backward rows: GE[NB] = 0, GE[t] = GE[t + 1] + ls_t; G[NB][n - 1] = 0, everything else -BIG; for t descending
 *     G[t][q] = (lps - stay_pen) + G[t + 1][q], then mx with lp[t][s[q + 1]] + G[t + 1][q + 1] (q + 1 < n), with
 *     (lp[t][s[q + 2]] - skip_pen) + G[t + 1][q + 2] (q + 2 < n), with -local_pen + GE[t + 1] (q == n - 1).
 *   An edit at base i keeps the first A = max(i - k + 1, 0) states of s, puts M >= 0 new states mid[0..M) behind them and continues with the
 *   suffix s[j0 ..] of Bn = n - j0 states; s' (n' states) are the edited sequence's.  A substitution: n' = n, j0 = min(i + 1, n); a deletion:
 *   n' = n - 1, j0 = min(i + 1, n); an insertion before i: n' = n + 1, j0 = min(i, n).  mid = s'[A .. n' - Bn), M <= k (0 for a deletion at
 *   i == 0), J = A + M the suffix's first index in s'.  Column idx of the edited lattice is F[.][idx] for idx < A and the edit's own
 *   Mc[.][idx - A] otherwise.
 *     1. Mc[0][m] = -BIG; Mc[t + 1][m] the cell rule at index A + m with state mid[m].
 *     2. Bn == 0: E = -BIG; per block E = mx(E + ls, col[t][J - 1] - local_pen); the score is base's end rule on (col[NB][J - 1], E).
 *     3. else per block t ascending, best = -BIG before: Y0, the arrival at index J from the step (J >= 1), then the skip (J >= 2), or from
 *        START (J == 0), with lp[t][s[j0]] and no stay; best = mx(best, Y0 + G[t + 1][j0]); where Bn >= 2 and J >= 1 also
 *        Y1 = (col[t][J - 1] - skip_pen) + lp[t][s[j0 + 1]], best = mx(best, Y1 + G[t + 1][j0 + 1]).
 *   A score below -BIG / 2 is NAN (no admissible path), as is every edit that leaves fewer than k bases.  sub[i][seq[i]] is computed as any other.
 * The join is exact: moves advance by 1 or 2, so a path reaches the suffix for the first time at exactly one block and in exactly one of its
 * first two states; before that block it lies in prefix and middle columns, from it on in the suffix's own cells, which the edit does not touch.
 * An edit's score and base are different chains of float32 additions: they agree to rounding, not in bits; a caller confirms the edits it
 * chooses with scrappie_hip_map_multi_batch, which is exact.
 *
 * scrappie_hip_map_edits_batch: reads[i] (prepared as for scrappie_hip_map_batch) against targets[i]: seq holds BASE codes 0..3 and seqlen
 * bases, unbanded; the engine encodes the k-mers.  out[i] as scrappie_hip_map_crf_edits_batch fills it (freed by
 * scrappie_hip_free_edits_results); base is not turned into NAN: it is scrappie_hip_map_batch's score as it is.  It runs as
 * scrappie_hip_map_batch does for a transducer: the network and S1 once per launch group, then k_map_edits_rows forward, k_map_edits_rows
 * backward and k_map_edits on the main stream while the posterior is resident.  A read adds its two row matrices
 * (scrappie_hip_map_edits_row_bytes) and its results to the cut into launch groups; the debug option "map_edits_budget_kb" bounds the row
 * and result bytes of one launch of the three kernels (0: one launch per launch group).  A target that cannot be scored -- no or an empty
 * sequence, fewer than k bases ("shorter than the model's k-mer"), a code that is not a base, poslow / poshigh set ("bands are not part of
 * this call"), more than scrappie_hip_map_edits_max_bases(k) bases ("too long for k_map_edits") -- gets base and every edit NAN and the first
 * such reason is the error text; its neighbours are scored.  A flip-flop (CRF) model: -1 with a text that names it and
 * scrappie_hip_map_crf_edits_batch.  viterbi 0: forward scores.  scrappie_hip_map_timing covers the call ([0] network + S1; [1] the three
 * launches with their copies; [2] stays 0); scrappie_hip_map_edits_timing has the kernels alone, as scrappie_hip_crf_edits_timing.
 *
 * map_post_edits: the same on a dense host log-posterior of nr = 4^k + 1 rows, k = 1 .. 5 (columns a multiple of 4 floats apart), and the
 * process-default engine, a batch of one; base, sub, del, ins may each be NULL; all are NAN, the return value 0 and the reason the error text
 * where the sequence cannot be scored.  -1 with the reason: a null argument, a posterior of another shape, a failed launch. */
int scrappie_hip_map_edits_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                 const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out);
int map_post_edits(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen, int viterbi,
                   float *base, float *sub, float *del, float *ins);
/* Host only (sh_host.c): what a launch of the three kernels keeps on the device.  pitch: floats from one entry's row to the next
 * (n + 1 = seqlen_bases - k + 2 rounded up to 16; 0 where there are fewer than k bases); row_bytes: the two row matrices of nblock + 1
 * entries; plan: reads in input order, rows[i] the float offset of read i's F in the row buffer (G (nblock[i] + 1) * pitch[i] floats behind
 * it), res[i] that of its results (sub [L][4], ins [L + 1][4], del [L]) in the result buffer, both multiples of 4; returns the floats of the
 * row buffer, *res_floats (may be NULL) those of the result buffer; -1, nothing written: k == 0 or a read of fewer than k bases.
 * max_bases: the longest sequence scored, scrappie_hip_map_lds_max_seq() states. */
size_t scrappie_hip_map_edits_pitch(size_t seqlen_bases, size_t k);
size_t scrappie_hip_map_edits_row_bytes(size_t seqlen_bases, size_t k, size_t nblock);
long long scrappie_hip_map_edits_plan(const size_t *seqlen, const size_t *nblock, size_t n, size_t k, int *pitch, long long *rows, long long *res,
                                      long long *res_floats);
size_t scrappie_hip_map_edits_max_bases(size_t k);
/* launches of each form in this process, all engines together: k_map_edits_rows at (viterbi ? 4 : 0) | (tiled ? 2 : 0) | (backward ? 1 : 0),
 * k_map_edits at 8 + ((viterbi ? 2 : 0) | (tiled ? 1 : 0)) */
void scrappie_hip_map_edits_form_counts(uint64_t forms[12]);
/* the last scrappie_hip_map_edits_batch call on this engine, as scrappie_hip_crf_edits_timing */
void scrappie_hip_map_edits_timing(scrappie_hip_engine *e, double ms[3], size_t *launches, size_t *row_bytes);

/* The same in a band (the kernels' banded forms, sh_map_edits.h): a read that covers a window lies on a narrow diagonal of the lattice, and rows,
 * traffic and sums are proportional to the cells visited.
 *
 * Definition (tests/test_map_edits_band_cpu.py restates it in numpy).  A band is what map_to_sequence_viterbi_banded / _forward_banded take: low,
 * high of nblock entries over the n = L - k + 1 states, valid iff are_bounds_sane(low, high, nblock, n).  Block t leads from entry t to entry
 * t + 1; cell q of entry t + 1 is admissible iff low[t] <= q < high[t].  Entry 0 has no cells, as above; START and END carry no band.  The
 * definition of scrappie_hip_map_edits_batch holds with these changes and no other:
 *   Rows.  F[t + 1][q] is the cell rule on the row of entry t where the cell is admissible and -BIG where it is not.  FS, the END chain, the end
 *     rule and base read those masked rows and are otherwise unchanged.  G[NB][n - 1] = 0 only where that cell is admissible.  G[t][q] for t >= 1
 *     is the unbanded recursion on the masked row of entry t + 1, and -BIG where cell q of entry t (band entry t - 1) is not admissible.  G[0]
 *     is never read.
 *   The edit's own M <= k middle columns Mc carry NO band: a band is given in the coordinates of the original sequence, and the new states have
 *     none there.
 *   The NAN rule and the sharing of the prefix's loads among the edits of a position are unchanged.
 * Consequences:
 *   Equivalence.  An edit's score is the score of the masked dynamic programme on the edited sequence in which cells idx < A keep the band of the
 *     original cell idx, the suffix's cells keep the band of their original index j0 + (idx - J), and the M middle cells are free at every entry.
 *   Full band.  With low[t] = 0 and high[t] = n at every block every output equals map_post_edits' bit for bit, Viterbi and forward: the banded
 *     forms run the same operations (sh_me_mx, sh_me_mx_if, sh_lse) on the same operands in the same order.
 *   A Viterbi band that contains the unbanded Viterbi path: base has the unbanded base's bits.
 *   base is NOT map_to_sequence_viterbi_banded / _forward_banded's score.  The reference's banded functions keep stale cells outside the band and
 *     assign two cells in block 0 from no source (sh_map.h describes it; k_map's banded form reproduces it literally and stays as it is); an edit
 *     cannot be defined on top of that.  The edits use the clean masked programme above.
 *   Identity substitution.  sub[i][seq[i]] is computed as any other substitution: its middle cells are free, so it may EXCEED base where the band
 *     binds on them.
 *   Ends.  A tight band can make edits at either end NAN -- the last positions where low[nblock - 1] == n: they close on cell n - 1 of entry
 *     nblock.  That is a result, not an error; the caller chooses the half-width.
 * Rows on the device: an entry's row holds its band's cells alone, cell q of entry t + 1 at float q - low[t], in rows of one pitch per read: the
 * widest entry's cells and one slot -- FS in the forward matrix, the stores of threads without a cell in the backward one -- rounded up to 16
 * floats (scrappie_hip_map_edits_band_pitch); two matrices of nblock + 1 such rows (scrappie_hip_map_edits_band_row_bytes).  The score rows of
 * k_map_edits_rows stay in LDS by k_map's formula, so the limit stays scrappie_hip_map_edits_max_bases(k).  k_map_edits walks, per workgroup of 64
 * or 256 positions (the default per form is the faster measured; the debug option "map_edits_band_width": 0 the default, 64, 256), only the blocks
 * at which one of its positions can have an admissible prefix source or a join.
 *
 * scrappie_hip_map_edits_banded_batch: as scrappie_hip_map_edits_batch (same results, same free function, the network once per launch group,
 * three launches); targets[i].poslow / poshigh hold nblock entries each for the read's nblock, or are both NULL: no band, run through the
 * unbanded forms in a launch of their own.  One of the two alone: "a band needs both poslow and poshigh".  A read's cost in the cut into launch
 * groups and under "map_edits_budget_kb" is its banded row bytes.  A band that is not valid for the read's block count and n (an array made for
 * another block count is not) gets NAN for that read and the first reason as the error text; its neighbours are scored.  A flip-flop (CRF)
 * model: -1.  scrappie_hip_map_edits_timing covers the call, row_bytes the bytes the launches kept.  scrappie_hip_map_edits_batch itself goes on
 * refusing bands.
 * map_post_edits_banded: a batch of one on a dense host log-posterior and the process-default engine, as map_post_edits; low and high are
 * required. */
int scrappie_hip_map_edits_banded_batch(scrappie_hip_engine *e, int model, const raw_table *reads, const scrappie_hip_map_target *targets, size_t n,
                                        const scrappie_hip_params *p, int viterbi, scrappie_hip_edits_result *out);
int map_post_edits_banded(const_scrappie_matrix logpost, float stay_pen, float skip_pen, float local_pen, const int *seq, size_t seqlen,
                          const size_t *low, const size_t *high, int viterbi, float *base, float *sub, float *del, float *ins);
/* Host only.  The band of half-width `halfwidth` states around a Viterbi path of k_map (path[t], t = 0 .. nblock - 1, as scrappie_hip_map_batch
 * and map_to_sequence_viterbi return it: the state after block t, -1 in START and END): with p[t] the position -- 0 over the leading START
 * entries, nstate - 1 over the trailing END entries -- low[t] = max(p - halfwidth, 0), high[t] = min(p + halfwidth + 1, nstate); low[0] = 0 and
 * high[nblock - 1] = nstate are forced; nblock entries each.  For every path it accepts the result passes are_bounds_sane and contains the path.
 * 0, or -1: a null or empty argument; halfwidth < 1 (a skip moves two states, so a half-width of 0 cannot pass are_bounds_sane); what is no path
 * of such a sequence -- a value outside -1 .. nstate - 1, a step down or above 2, a -1 between positions, no position at all, a first position
 * other than 0, a last other than nstate - 1. */
int scrappie_hip_map_path_band(const int *path, size_t nblock, size_t nstate, size_t halfwidth, size_t *low, size_t *high);
/* Host only (sh_host.c), as scrappie_hip_map_edits_pitch / _row_bytes / _plan for reads in bands: pitch, the floats of an entry's row (0: a null
 * argument); row_bytes, the two matrices; plan, with low[i] / high[i] read i's band of nblock[i] entries (either NULL: the read has none and takes
 * the unbanded pitch). */
size_t scrappie_hip_map_edits_band_pitch(const size_t *low, const size_t *high, size_t nblock);
size_t scrappie_hip_map_edits_band_row_bytes(const size_t *low, const size_t *high, size_t nblock);
long long scrappie_hip_map_edits_band_plan(const size_t *seqlen, const size_t *nblock, const size_t *const *low, const size_t *const *high, size_t n,
                                           size_t k, int *pitch, long long *rows, long long *res, long long *res_floats);
/* launches of each banded form in this process: [0 .. 8) k_map_edits_rows indexed as scrappie_hip_map_edits_form_counts (which counts the unbanded
 * forms alone), [8 .. 12) k_map_edits at 256 positions per workgroup and [12 .. 16) at 64, each at (viterbi ? 2 : 0) | (tiled ? 1 : 0) */
void scrappie_hip_map_edits_band_form_counts(uint64_t forms[16]);
/* private (scratch) bytes per lane of each banded form, as the runtime reports them for the loaded kernels, indexed as the form counts (needs a
 * device; -1: the runtime gave no answer).  The forms are built to need none. */
void scrappie_hip_map_edits_band_scratch(long long bytes[16]);

/* Squiggle matching, batched (sh_eng_squig.inc): reads[i] (trimmed, normalised; mapped over [start, end)) against
 * targets[i], a predicted squiggle of npos columns of stride >= 3 floats (mean, log sd, dwell logit); out[i] belongs to
 * reads[i].  No network runs and no model is needed (the squiggles are an input here: scrappie_hip_squiggle_predict_batch
 * makes them).  viterbi 0: forward scores.  want_path (Viterbi only): out[i].path
 * is the reference's path_padded, malloc'd, out[i].n = reads[i].n int32.  The call is cut into launches whose
 * traceback (samples x positions / 2 bytes per read) and scratch fit half of the device memory that is free; a single
 * read that does not fit gets NAN and an error text, as does one the per-read functions refuse, and the others are
 * untouched.  p NULL: scrappie_hip_default_squiggle_params() (scrappy's defaults); an invalid rate or prob_back fails the
 * call.  Returns 0, or -1 with scrappie_hip_last_error() when the call as a whole fails.  A launch holds the engine's lock. */
typedef struct { const float *params; size_t npos, stride; } scrappie_hip_squiggle_target;
typedef struct { float rate, prob_back, local_pen, skip_pen, minscore; } scrappie_hip_squiggle_params;
typedef struct { float score; size_t n; int32_t *path; } scrappie_hip_squiggle_result;
scrappie_hip_squiggle_params scrappie_hip_default_squiggle_params(void);
int scrappie_hip_squiggle_match_batch(scrappie_hip_engine *e, const raw_table *reads, const scrappie_hip_squiggle_target *targets, size_t n,
                                      const scrappie_hip_squiggle_params *p, int viterbi, int want_path, scrappie_hip_squiggle_result *out);
void scrappie_hip_free_squiggle_results(scrappie_hip_squiggle_result *r, size_t n);
/* the last scrappie_hip_squiggle_match_batch call's time, milliseconds summed over its launches: [0] tables on the host +
 * uploads, [1] k_squig, [2] k_squig_walk + results to the host (host clock, the stream drained between the stages) */
void scrappie_hip_squiggle_timing(scrappie_hip_engine *e, double out[3]);
/* positions up to which k_squig keeps its score rows and tables in LDS; longer squiggles keep the rows in device scratch */
size_t scrappie_hip_squiggle_lds_max_pos(void);
/* The planners' scratch arithmetic on the host, no device (for the tests): reads of seqlen[i] states / npos[i] positions laid
 * out in this order in one launch; off[i] = float offset of read i's two score rows in the launch's scratch allocation (-1: the
 * rows live in LDS); returns the floats allocated for all of them.  k_map touches 2 (seqlen + 2) floats from its offset,
 * k_squig 2 (2 npos + 1). */
long long scrappie_hip_map_plan_scratch(const size_t *seqlen, const size_t *nblock, size_t n, long long *off);
long long scrappie_hip_squiggle_plan_scratch(const size_t *npos, const size_t *nsample, size_t n, long long *off);
/* Banded squiggle matching (sh_squig_band.h).  bands[i] is read i's band as squiggle_match_viterbi_banded takes it (low: one
 * int32 per sample of the window; it may differ from read to read), low NULL and width 0 for a read without one; bands NULL: no
 * read has one, which is scrappie_hip_squiggle_match_batch.  Banded reads go through k_squig_band in launches of their own, the
 * others through k_squig as ever.  A banded read costs a launch samples x width / 2 bytes of traceback and, beyond
 * scrappie_hip_squiggle_band_lds_max_width(), 2 (2 width + 1) floats of scratch: one that is refused for its size without a band
 * may fit with one.  An invalid band, or one that admits no path (score below -1e30 / 2): NAN, no path and an error text for that
 * read, the others untouched.  scrappie_hip_squiggle_timing covers these calls too. */
typedef struct { const int32_t *low; size_t width; } scrappie_hip_squiggle_band;
int scrappie_hip_squiggle_match_banded_batch(scrappie_hip_engine *e, const raw_table *reads, const scrappie_hip_squiggle_target *targets,
                                             const scrappie_hip_squiggle_band *bands, size_t n, const scrappie_hip_squiggle_params *p, int viterbi,
                                             int want_path, scrappie_hip_squiggle_result *out);
/* the diagonal band of half-width h positions: returns width = min(npos, 2 h + 1) and fills low[t] =
 * clamp(floor(t npos / nsample) - h, 0, npos - width), t < nsample (64-bit arithmetic); low NULL: the width alone */
size_t scrappie_hip_squiggle_diagonal_band(size_t nsample, size_t npos, size_t halfwidth, int32_t *low);
/* the widest band whose score rows k_squig_band keeps in LDS; wider bands keep them in device scratch */
size_t scrappie_hip_squiggle_band_lds_max_width(void);
/* The banded planner's arithmetic on the host, no device (for the tests): banded reads laid out in this order in one launch;
 * scr_off[i] the float offset of read i's rows (2 (2 width + 1) floats; -1: in LDS), tb_off[i] its first traceback word
 * (nsample x 8 ceil(width / 64) words, then nsample int32 of END's source; -1 without want_path), scr_off[n] / tb_off[n] the
 * floats / words allocated for all (arrays of n + 1, either may be NULL); width[i] > npos[i] counts as npos[i].  Returns the
 * device bytes the launch is charged. */
long long scrappie_hip_squiggle_band_plan(const size_t *npos, const size_t *width, const size_t *nsample, size_t n, int want_path,
                                          long long *scr_off, long long *tb_off);
/* launches of each k_squig_band form in this process: index (viterbi ? 2 : 0) | (scratch ? 1 : 0) */
void scrappie_hip_squiggle_band_form_counts(uint64_t forms[4]);
/* One signal against many candidate squiggles, unbanded (sh_squig_pack.h, sh_eng_squig_pack.inc): which of these squiggles does
 * this signal fit best?  cands[i] holds read i's candidates; a cand array that several reads point at is checked, turned into
 * tables and packed once, and uploaded once per launch.  A read's signal is uploaded once; its candidates are laid end to end
 * into packs, every pack of every read of a launch a workgroup of one k_squig_pack launch; a candidate too long for a pack,
 * or left alone in its pack (unless the debug option "squig_pack_lone" is 1), goes through k_squig in the same call.  out[i].score[k] (malloc'd, ncand floats) is the raw squiggle_match_viterbi / _forward
 * score of (reads[i], cands[i].cand[k]) -- in Viterbi the bits scrappie_hip_squiggle_match_batch gives for that pair --; START
 * and END absorb what a candidate leaves of the window, so candidates of different lengths compare as they are.  best: the
 * highest finite score, the lowest index on a tie, -1: none.  With viterbi and want_path, path (malloc'd, n entries) is the
 * best candidate's path_padded, from a second pass of k_squig / k_squig_walk on that pair alone.  A candidate with no params, no
 * positions, a stride below 3 or more than the longest squiggle mapped gets NAN and its neighbours are scored; a read that
 * fails its own checks or fits no launch gets every score NAN and best -1, the others untouched; the first such reason is the
 * error text, the return 0.  An invalid rate or prob_back, or a failed launch, fails the call (-1, out[] freed and blanked).
 * scrappie_hip_squiggle_timing covers these calls too. */
typedef struct { const scrappie_hip_squiggle_target *cand; size_t ncand; } scrappie_hip_squiggle_candidates;
typedef struct { float *score; size_t ncand; int best; size_t n; int32_t *path; } scrappie_hip_squiggle_multi_result;
int scrappie_hip_squiggle_match_multi_batch(scrappie_hip_engine *e, const raw_table *reads, const scrappie_hip_squiggle_candidates *cands,
                                            size_t n, const scrappie_hip_squiggle_params *p, int viterbi, int want_path,
                                            scrappie_hip_squiggle_multi_result *out);
void scrappie_hip_free_squiggle_multi_results(scrappie_hip_squiggle_multi_result *r, size_t n);
/* the same for one read on the process-default engine, scores only: score[ncand]; p NULL: the defaults.  0, or -1 */
int scrappie_hip_squiggle_match_multi(const raw_table signal, const scrappie_hip_squiggle_target *cand, size_t ncand,
                                      const scrappie_hip_squiggle_params *p, int viterbi, float *score);
/* The packing on the host, no device.  Candidates of npos[k] positions (a cell each) into packs of at most pack_cells cells (at
 * most scrappie_hip_squiggle_pack_max_cells(), which follows from the LDS a cell, a candidate and an END piece take), in input
 * order: a pack closes when the next candidate would take it past pack_cells.  pack[k]: the candidate's pack, cell[k]: its first
 * cell there; -1 both where the candidate has more positions than a pack may hold (it takes k_squig) or none.  Returns the
 * number of packs.  The debug option "squig_pack_cells" sets an engine's pack_cells (0: every candidate through k_squig, one
 * workgroup each; -1: the default; a NULL engine: the process-default engine). */
long scrappie_hip_squiggle_pack_plan(const size_t *npos, size_t ncand, size_t pack_cells, int *pack, long long *cell);
size_t scrappie_hip_squiggle_pack_max_cells(void);
/* pack `which` of that plan as k_squig_pack reads it: per cell of the pack wa (position in its candidate | the candidate's index
 * in the pack << 12 | 1 << 24 position 0 | 1 << 25 position 1 | 1 << 26 position <= npos - 2) and wb (its END piece | 1 << 30 on
 * the piece's first cell); per candidate of the call piece0[k] / npiece[k], its pieces in the pack (untouched for candidates of
 * other packs).  A piece is a candidate's cells inside one group of 64 consecutive cells.  Any array may be NULL.  Returns the
 * pack's pieces. */
size_t scrappie_hip_squiggle_pack_layout(const size_t *npos, size_t ncand, const int *pack, int which, int *wa, int *wb, int *piece0,
                                         int *npiece);
/* launches of each k_squig_pack form in this process: index viterbi (0: forward, 1: Viterbi) */
void scrappie_hip_squiggle_pack_form_counts(uint64_t forms[2]);
/* A raw signal mapped INTO a longer reference squiggle (k_squig_local, sh_squig_local.h; sh_eng_squig_local.inc): where in the
 * reference does this signal lie?  Not in the reference project.  The definition is squiggle_match_viterbi / _forward with the
 * squiggle side made local: the move out of START enters at EVERY position and one END accumulator per position lets every
 * position leave, both without a distance term; START and END still absorb samples at local_pen each; START has no step or skip
 * of its own; the score is the best of the last row's position cells and END accumulators (Viterbi), or their log-sum.  The
 * score is never below squiggle_match_viterbi's for local_pen >= 0, and with local_pen = 0 and a path that ends in END it is
 * squiggle_match_viterbi's bit for bit.  The reference is cut into windows by the entry position of a path, one workgroup each; the
 * Viterbi score has the same bits for every cut.
 * Batched: out[i] belongs to (reads[i], targets[i]); a target that several reads point at (the same params, npos and stride) is
 * checked once per call, goes through the table computation once per call and is uploaded once per launch.  score; n = reads[i].n;
 * with viterbi: last = the end cell's position + 1; with viterbi and want_path also first, the lowest position on the path, and
 * path (n entries, malloc'd; scrappie_hip_free_squiggle_local_results): positions in the reference's coordinates, -1 in START, END
 * and outside [start, end), back states as their position.  Otherwise first = (size_t)-1, last = 0, path = NULL.  A read whose
 * checks fail, or that fits no launch ("squiggle_budget_kb"), gets NAN and an error text, the others are untouched.  Returns 0, or
 * -1 when the call as a whole fails (then every score is NAN).  scrappie_hip_squiggle_timing covers these calls too: [0] tables +
 * uploads, [1] the first pass, [2] the second pass, the walk and the results. */
typedef struct { float score; size_t first, last, n; int32_t *path; } scrappie_hip_squiggle_local_result;
int scrappie_hip_squiggle_match_local_batch(scrappie_hip_engine *e, const raw_table *reads, const scrappie_hip_squiggle_target *targets,
                                            size_t n, const scrappie_hip_squiggle_params *p, int viterbi, int want_path,
                                            scrappie_hip_squiggle_local_result *out);
void scrappie_hip_free_squiggle_local_results(scrappie_hip_squiggle_local_result *r, size_t n);
/* the same for one read on the process-default engine, with squiggle_match_viterbi's arguments: path_padded (signal.n entries),
 * first and last may each be NULL; NAN and an error text where squiggle_match_viterbi gives them */
float squiggle_match_local_viterbi(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                   float skip_pen, float minscore, int32_t *path_padded, size_t *first, size_t *last);
float squiggle_match_local_forward(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                                   float skip_pen, float minscore);
/* The cut into windows on the host, no device.  stride: entry positions per window; 0: one window; < 0: the default.  Window w owns
 * the entry positions [w s, min((w + 1) s, npos)) (own[w] of them) and holds the cells first[w] = max(w s - 1, 0) ..
 * min(w s + s - 1 + 2 (nsample - 1), npos - 1) (ncell[w]); home[w]: 0 rows and tables in LDS (at most
 * scrappie_hip_squiggle_local_max_cells() cells: (16 + 10 ncell + 2) * 4 bytes within 64 KiB), 1 rows in device scratch at float
 * offset scr_off[w] of *scr_floats in all (5 ncell per window, rounded up to a multiple of 4).  Arrays may be NULL; only the first
 * cap windows are written.  Returns the number of windows; 0: nothing to cut.  The debug option "squig_local_stride" sets an
 * engine's stride (a NULL engine: the process-default engine). */
long long scrappie_hip_squiggle_local_plan(size_t npos, size_t nsample, long stride, size_t cap, size_t *first, size_t *ncell, size_t *own,
                                           int *home, long long *scr_off, long long *scr_floats);
size_t scrappie_hip_squiggle_local_stride(size_t npos, size_t nsample, long stride);
size_t scrappie_hip_squiggle_local_max_cells(void);
/* launches of each k_squig_local form in this process: index (viterbi ? 2 : 0) | (scratch ? 1 : 0) */
void scrappie_hip_squiggle_local_form_counts(uint64_t forms[4]);
/* Squiggle prediction, batched (sh_eng_sqnet.inc): seqs[i] holds n[i] bases coded 0..3; out[i] becomes a matrix as
 * squiggle_r94 returns it (free_scrappie_matrix), predicted with `model`, a squiggle model loaded on e under that name.
 * The accepted sequences are laid end to end: one upload, one k_sqnet launch over all their tiles, one download; the call
 * is cut into several such launches where codes and outputs (13 bytes per base) exceed half of the device memory that is
 * free.  A sequence the per-read functions refuse, or one that alone exceeds a launch, gets out[i] = NULL and an error
 * text, and the others are untouched.  Returns 0, or -1 with scrappie_hip_last_error() when the call as a whole fails
 * (then every out[i] is NULL).  A launch holds the engine's lock. */
int scrappie_hip_squiggle_predict_batch(scrappie_hip_engine *e, const char *model, const int *const *seqs, const size_t *n, size_t count,
                                        int transform_units, scrappie_matrix *out);
/* the last scrappie_hip_squiggle_predict_batch call's time, milliseconds summed over its launches: [0] staging + upload,
 * [1] k_sqnet, [2] download + transform (host clock, the stream drained between the stages) */
void scrappie_hip_sqnet_timing(scrappie_hip_engine *e, double out[3]);
/* output positions per workgroup of k_sqnet (host only, no device): sequences longer than this span several tiles */
size_t scrappie_hip_sqnet_tile(void);
/* launches of k_sqnet since the process started, all engines together (a host counter) */
uint64_t scrappie_hip_sqnet_launch_count(void);

/* Base probabilities of the flip-flop (CRF) models, batched (k_crf_post, sh_crf_post.h; sh_eng_crfpost.inc): the forward / backward pass of
 * posterior_crf (src/decode.c:928) over a read's normalised transitions on the device, 8 lanes per read.  A result is the 5 x (nblock + 1)
 * matrix posterior_crf returns -- rows A, C, G, T, stay; every column total carries the reference's extra e^0, so a column sums to less than
 * one -- malloc'd, the caller's to free_scrappie_matrix.
 * The per-read symbol posterior_crf (and scrappy's basecall_raw(..., with_base_probs=True) on top of it) stays the host function: it is pinned
 * bit for bit against the compiled reference, whose log-sum-exp is libm's log1pf(expf()); the device's is the transcendental unit's, within a
 * few ulp of a correction term of at most log 2 per step, and cannot keep that promise.  The functions below agree with it to rounding. */
/* Host only: off[i] = float offset of read i's (nblock[i] + 1) x 5 floats in a launch's output buffer, reads end to end in this order, every
 * start 16-byte aligned, nothing for a read without blocks; returns the floats of all of them (-1: a null argument).  Neighbouring reads are
 * written by different workgroups and a result cannot show an overlap, so the plan is open to the tests. */
long long scrappie_hip_crf_post_plan(const size_t *nblock, size_t n, long long *off);
/* trans[i]: 25 rows (from state minor, to state major; ACGT-), nc >= 1 blocks, as nanonet_rnnrf_r94_transitions returns it.  The accepted
 * matrices go up end to end: one upload, one launch of k_crf_post, one download; a call of more than 4 000 000 blocks is cut into several.
 * A NULL or misshapen matrix gets out[i] = NULL and an error text, the others are untouched.  Returns 0, or -1 with
 * scrappie_hip_last_error() when the call as a whole fails (out[] is then all NULL). */
int scrappie_hip_posterior_crf_batch(scrappie_hip_engine *e, const const_scrappie_matrix *trans, size_t n, scrappie_matrix *out);
/* scrappie_hip_basecall_batch for a CRF model (any other: -1) that returns the base probabilities as well: out[] is exactly what
 * scrappie_hip_basecall_batch gives for the same input; probs[i] is read i's 5 x (nblock + 1) posterior, NULL where the read has no call.
 * Inside a launch group k_crf leaves the normalised transitions on the device, k_crf_post runs behind it on the main stream, and the
 * probabilities come back on the copy stream behind the group's calls: 20 bytes per block.  Failures as scrappie_hip_basecall_batch (a failed
 * call returns nothing).  The call runs alone: it does not share launch groups with concurrent small calls, and keeps chain-bound reads on
 * this engine. */
int scrappie_hip_basecall_batch_probs(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n, const scrappie_hip_params *p,
                                      scrappie_hip_call *out, scrappie_matrix *probs);
/* the last of the two calls above, milliseconds summed over its launch groups.  scrappie_hip_basecall_batch_probs: [0] network + k_crf,
 * [1] k_crf_post, [2] the probabilities' transfer to the host (device events; nothing waits for them while the groups run).
 * scrappie_hip_posterior_crf_batch: [0] staging + upload, [1] k_crf_post, [2] download + results (host clock, the stream drained between). */
void scrappie_hip_crf_post_timing(scrappie_hip_engine *e, double out[3]);
/* launches of k_crf_post since the process started, both forms and all engines together (a host counter) */
uint64_t scrappie_hip_crf_post_launch_count(void);
/* Launches of each kernel form since the process started, all engines together (the per-read functions run on the
 * process-default engine).  map_forms[(viterbi ? 8 : 0) | (banded ? 4 : 0) | (tiled ? 2 : 0) | (scratch ? 1 : 0)] for k_map,
 * squig_forms[(viterbi ? 2 : 0) | (scratch ? 1 : 0)] for k_squig; either may be NULL.  Host counters only: no device work. */
void scrappie_hip_launch_form_counts(uint64_t map_forms[16], uint64_t squig_forms[4]);

/* Measurement / test hook for SURVEY.md 8(d) "decode driven by HMM-simulated posteriors" (synthetic
 * weights decode to a handful of bases per read, which leaves the decode -> D2H -> homopolymer ->
 * overlapper stage almost idle).  From the next launch group on, everything downstream of S1 -- the
 * device Viterbi, the homopolymer rows, scrappie_hip_posterior -- sees, instead of the network's own
 * normalised posterior, probabilities supplied by the caller: read i of a launch group takes the
 * row-major [nblock_i][nstate] float matrix at d_prob + prob_off[i % n_prob] (DEVICE memory, nstate =
 * the model's; rows past the read's nblock are not read).  The network itself still runs in full (S1
 * writes its own buffer).  The decoder image of the matrices is built on the first launch group and
 * re-used while consecutive groups have the same shape.  d_prob = NULL switches the hook off.
 * Transducer models only; no launch group may be in flight.  The reference has no counterpart. */
int scrappie_hip_set_decoder_input(scrappie_hip_engine *e, const float *d_prob, const uint64_t *prob_off, size_t n_prob);

/* The same idea one stage earlier, so that the DEFAULT decode path (S1 inside the decoder, k_ff_viterbi) sees
 * realistic posteriors: from the next launch group on, the output layer (S1 / globalnorm) and everything
 * downstream read, instead of the trunk's own output, activations supplied by the caller: read i of a launch
 * group takes the row-major [nblock_i][S] float matrix at d_trunk + trunk_off[i % n_trunk] (DEVICE memory, S = the
 * model's state width; blocks past the matrix's read are zero).  The network above the output layer still runs
 * in full.  With an output layer built from state codes (scrappie_amd.synth.hmm_output_layer) the posteriors
 * are those of a simulated k-mer path, computed by the production kernels.  d_trunk = NULL switches the hook
 * off; no launch group may be in flight.  The reference has no counterpart. */
int scrappie_hip_set_trunk_input(scrappie_hip_engine *e, const float *d_trunk, const uint64_t *trunk_off, size_t n_trunk);

/* Test hooks (tests/test_gpu_parity.py: the whole traceback of the two decoder forms, byte for byte).
 * scrappie_hip_debug_option: "ff_separate" = S1 and the decoder as two kernels on this engine (k_ff_lds / k_ff_exp +
 * k_viterbi) even where the one-kernel forms apply; "fv_single" = S1 inside the decoder on k_ff_viterbi's eight do-everything waves
 * instead of k_ff_viterbi_teams (S1 team + decoder team; env SH_FV_SINGLE=1 does the same for a process); "dump_final" = the decoders leave every tile's final scores in the
 * hand-over buffer; "fail_run" = k: the k-th next launch group is refused (failure paths); "redo_all" = every read
 * takes the host fallback of k_stitch; "gru_tiles" = 1 / 2: tiles of 16 reads per workgroup of the recurrent layers
 * whatever the lane schedules say (0: the engine chooses); "decoder_cus" = n: the decoder's piece schedule is made for a device of n CUs (with
 * 2, a group of three or more tiles is cut into two pieces a tile and the pieces' hand-over runs on a small group; 0: the device's own count) --
 * for all three decoder forms, the two-team kernel then running one piece per workgroup like the other two; "decoder_lanes" = n: the
 * two-team kernel's lane layout (sh_decoder_lanes) is made for a device of n CUs, so a group of a few tiles runs on n workgroups that walk
 * several segments each and hand cut tiles over (0: the device's own count; it goes before "decoder_cus" for that kernel).
 * scrappie_hip_debug_fetch copies a buffer of the most recent transducer launch group to the
 * host: "tb" (one byte per state: [column block][state quad][read of tile][state of quad]), "tb_end" (int per
 * column block and read), "final_state" / "final_score" (per read, tiled order), "final_scores" ([tile][states x
 * 16 reads | 16 start | 16 end] floats, needs dump_final), "order" (int per tiled position: index of the read in
 * the call, -1 = padding), "tile_boff" (long long per tile: its first column block), "n_redo" (unsigned long long:
 * reads whose stitching k_stitch has left to the host since the engine was created), "gru_tiles" (int: what the group's
 * recurrent layers ran with), "decoder_pieces" (int: the segments of tiles the group's decoder launch ran: one per workgroup for k_viterbi and
 * k_ff_viterbi, which own a piece of a tile each, and all the segments of the lane layout for k_ff_viterbi_teams, whose workgroups walk several),
 * "decoder_wgs" (int: the workgroups of that launch).  Returns the bytes the
 * buffer holds (min(that, nbytes) are copied; dst may be NULL), -1 on error. */
int scrappie_hip_debug_option(scrappie_hip_engine *e, const char *name, int value);
/* k_stitch (homopolymer correction + k-mer stitching / crfpath_to_basecall on the device: what the batched path
 * runs instead of src/homopolymer.c:175 + src/decode.c:449 / :895 on the host) on ONE read given on the host, for
 * the bit-exact tests against the compiled-reference fixtures.  path: nblock + 1 entries; side: [nblock][5] log-
 * posterior rows (homopolymer k-mers of A, C, G, T, then stay) or NULL (no homopolymer pass); nstate: 4^k + 1 (25
 * with crf != 0).  bases takes at most cap bytes incl. the NUL; pos (nblock + 1 ints) and redo (1: the device
 * left the posterior-mean rounding of a run to the host) may be NULL.  Returns the number of bases, -1 = no
 * call (all stays), -2 = error. */
long scrappie_hip_debug_stitch(scrappie_hip_engine *e, const int *path, const float *side, size_t nblock, int nstate, int crf,
                               char *bases, size_t cap, int *pos, int *redo);
long long scrappie_hip_debug_fetch(scrappie_hip_engine *e, const char *what, void *dst, size_t nbytes);
/* k_stitch_dwell (sh_dwell.h: the dwell-corrected stitching of the events path on the device) on a batch of reads given on the host,
 * for the bit-exact tests against the compiled-reference fixtures; one launch, 64 reads to a wave.  Read i: nentry[i] events, its
 * path of nentry[i] + ntrail entries (ntrail 0 or 1; the engine runs with 1) and its nentry[i] dwells end to end in paths / dwells,
 * prior_num[i] (the last event's length + (float)(the span of the starts)), cap[i] bytes of the device's bases buffer (rounded up to
 * 16; scrappie_hip_dwell_capacity is what the engine reserves), the reads' reservations end to end.  bases takes that whole buffer as the
 * device leaves it (bases_off[i]: where read i's begins; both sized by the caller from the rounded caps), lengths[i] the bases
 * (-1: no call; 0 with redo[i] = 1: the read did not fit cap[i] and is the host's), pos (may be NULL) overlapper's pos[], laid out like
 * paths.  Returns 0, -1 on error. */
int scrappie_hip_debug_stitch_dwell(scrappie_hip_engine *e, const int *paths, const int *dwells, const size_t *nentry, size_t nread, int ntrail,
                                    const float *prior_num, int nstate, const size_t *cap, char *bases, size_t bases_bytes, int *lengths, int *pos,
                                    int *redo);
/* The cut of the split products (sh_kernels.h: split8, which every kernel's activations go through) on n values given on the host, for
 * the bit-exact test of the device's cut against its definition: p1[i] = fp16(64 x[i]), p2[i] = fp16(64 x[i] - p1[i]), as fp16 bit
 * patterns (n each).  Values are taken in groups of eight, the last group filled with zeros.  Returns 0, -1 on error. */
int scrappie_hip_debug_split(scrappie_hip_engine *e, const float *x, size_t n, uint16_t *p1, uint16_t *p2);
/* One activation form of the kernels (sh_kernels.h) on n values given on the host, in one kernel, for the tests that hold the forms to each
 * other bit for bit and to float64 where network weights do not reach: deep saturation, the clamp of the exponential, signed zeros,
 * subnormals.  The *_ACC forms take their argument as the split products leave it, in accumulator units: 2^14 x (exact in fp32).  Values
 * are taken in groups of four, the last group filled with zeros.  Returns 0, -1 on error. */
enum {
    SH_GATE_LOGISTIC = 0,           /* d_logistic */
    SH_GATE_TANH = 1,               /* d_tanh */
    SH_GATE_LOGISTIC4 = 2,          /* d_logistic4 */
    SH_GATE_TANH4 = 3,              /* d_tanh4 */
    SH_GATE_LOGISTIC4_ACC = 4,      /* d_logistic4_acc */
    SH_GATE_TANH4_ACC = 5,          /* d_tanh4_acc */
    SH_GATE_EXP = 6,                /* d_exp */
    SH_GATE_EXP_ACC = 7,            /* d_exp_acc */
    SH_GATE_EXP_ACC_INRANGE = 8,    /* d_exp_acc_inrange: only for |x| < 88 */
    SH_GATE_ELU = 9,                /* d_elu */
    SH_GATE_NFORM = 10
};
int scrappie_hip_debug_gates(scrappie_hip_engine *e, int which, const float *x, size_t n, float *out);
/* bytes of bases the engine reserves for a read whose path has nentry entries when the dwell correction is on */
size_t scrappie_hip_dwell_capacity(size_t nentry);

/* Posterior of one read on a given engine/model (what the per-read surface
 * calls): HOST matrix in reference layout. */
scrappie_matrix scrappie_hip_posterior(scrappie_hip_engine *e, int model, const raw_table signal,
                                       float min_prob, float tempW, float tempb, bool return_log);
/* Intermediate activations for layer-by-layer parity tests: layer 0 = conv +
 * activation, 1..5 = GRU layer outputs (incl. residual for rnnrf). */
scrappie_matrix scrappie_hip_trunk(scrappie_hip_engine *e, int model, const raw_table signal, int upto);

/* Events models (arch "events"): the input of a read is its windowed feature matrix,
 * row-major [nevent][12] floats.  For these models the raw_table / offsets / lengths of the
 * calls above count FLOATS of that matrix for `raw`, `start`, `end` and offsets, and EVENTS
 * for `lengths` of scrappie_hip_run_device.
 * scrappie_hip_event_features: events[start..end) -> out[(end-start) * 12]
 *   = window(nanonet_features_from_events(events, true), 3, 1)   (networks.c:155-157). */
int scrappie_hip_event_features(const event_table events, float *out);
scrappie_matrix scrappie_hip_events_posterior(scrappie_hip_engine *e, int model, const float *feature3, size_t nevent,
                                              float min_prob, float tempW, float tempb, bool return_log);

/* Event detection, batched (sh_eng_events.inc, kernels in sh_events.h): detect_events for every reads[i].raw[start .. end) in one call.
 * results[i].events belongs to reads[i]: .event malloc'd (scrappie_hip_free_event_results), NULL with status 1 where the read has no
 * peak (the reference is undefined there), status 2 where the read was refused (no signal, an empty window, more samples than one launch
 * may hold; the first such reason is the call's error text).  p NULL: event_detection_defaults.  The reads are sorted by length and cut
 * into launches under a sample budget (28 bytes of device scratch per sample + the signal; half of the free device memory, or the debug
 * option "events_budget_samples").  Returns 0, or -1 with scrappie_hip_last_error() when the call as a whole fails (then every table is
 * NULL).  A launch holds the engine's lock.  Bit-identical to scrappie_hip_detect_events_host, and so to the reference. */
typedef struct { event_table events; int status; } scrappie_hip_event_result;
int scrappie_hip_detect_events_batch(scrappie_hip_engine *e, const raw_table *reads, size_t n, const detector_param *p,
                                     scrappie_hip_event_result *results);
void scrappie_hip_free_event_results(scrappie_hip_event_result *r, size_t n);
/* the last scrappie_hip_detect_events_batch call's time, milliseconds summed over its launches: [0] staging + upload, [1] the four
 * kernels, [2] event tables to the host (host clock, the stream drained between the stages) */
void scrappie_hip_event_timing(scrappie_hip_engine *e, double out[3]);
/* samples per read of one staged tile of the serial kernels (host only): reads longer than this take several tiles */
size_t scrappie_hip_event_tile(void);
/* launches of scrappie_hip_detect_events_batch since the process started, all engines together (a host counter; tests) */
uint64_t scrappie_hip_event_launch_count(void);
/* The planner's arithmetic on the host, no device (for the tests).  Reads of nsample[i] samples laid out in this order in one launch:
 * off[i] = the first slot of read i, which owns nsample[i] + 1 slots from there in each of the five scratch arrays (running sums and
 * sums of squares: double; the two statistics: float; peaks: uint32; 28 bytes per slot); returns the slots of the launch. */
long long scrappie_hip_events_plan_scratch(const size_t *nsample, size_t n, long long *off);
/* ... and the cut of a call into launches of at most budget_slots slots: order[] takes the read indices sorted by length, longest
 * first; starts[] the first position (in that order) of each launch; returns the number of launches (even if > cap), -1 if one read
 * alone exceeds the budget. */
long scrappie_hip_events_plan_launches(const size_t *nsample, size_t n, size_t budget_slots, uint32_t *order, size_t *starts, size_t cap);
/* `scrappie events` for a batch (scrappie_events.c:271-330): batched event detection (p NULL: event_detection_defaults), the features
 * of each read on host threads (scrappie_hip_event_features; they stay on the host: the reference studentises with rsqrtps, whose bits
 * are the CPU's own), the launch groups of the events model `model` with the homopolymer pass off and -- dwell_correction != 0 -- the
 * stitching in dwell mode (sh_dwell.h), the calls in input order.  reads: pA, windows already trimmed.  out[i].nblock is the number of
 * events; a read without events or without a k-mer has no call (basecall NULL).  params NULL: scrappie_hip_default_params (its
 * homopolymer field is ignored).  Returns 0, -1 on error (nothing is returned then). */
int scrappie_hip_basecall_events_batch(scrappie_hip_engine *e, int model, const raw_table *reads, size_t n, const detector_param *p,
                                       const scrappie_hip_params *params, int dwell_correction, scrappie_hip_call *out);
/* The host statement of detect_events (sh_host.c) on x[0 .. n): what the kernels are held against bit for bit (tests, tools; the
 * per-read surface never falls back to it: without a device detect_events fails).  .event NULL where there is no peak.  tstat1 / tstat2 (may be NULL): n floats each, the two statistics. */
event_table scrappie_hip_detect_events_host(const float *x, size_t n, const detector_param *p, float *tstat1, float *tstat2);

/* Lane schedule of the recurrent kernel (scrappie_amd/csrc/sh_sched.h), host only:
 * how the tiles (16 reads, tile_T[i] blocks) of a launch group are cut into
 * segments for the 2 * nwg lanes.  lane_off: 2 * ncu + 1 ints; seg: cap rows of
 * {tile, first step, end step, 0}.  Returns the number of segments. */
long scrappie_hip_gru_schedule(const int *tile_T, size_t ntile, int ncu, int *nwg, int *capacity,
                               int *lane_off, int *seg, size_t cap);
/* ... with lanes_per_wg = 1 (k_gru_proj: projection + recurrence teams, one lane per workgroup) or 2;
 * lane_off: lanes_per_wg * ncu + 1 ints */
long scrappie_hip_lane_schedule(const int *tile_T, size_t ntile, int ncu, int lanes_per_wg, int *nwg, int *capacity,
                                int *lane_off, int *seg, size_t cap);

/* Pieces of the Viterbi decoder's launch (scrappie_amd/csrc/sh_sched.h), host only:
 * seg takes cap rows of {tile, first block, end block, 0} in workgroup order. */
long scrappie_hip_decoder_pieces(const int *tile_T, size_t ntile, int ncu, int *seg, size_t cap);
/* Lane layout of the two-team decoder (k_ff_viterbi_teams; sh_decoder_lanes in sh_sched.h), host only: the tiles end to end over one
 * lane per workgroup, nwg = min(ncu, live tiles) workgroups, cut only where a lane is full and only on even blocks.  lane_off: ncu + 1
 * ints; seg: cap rows of {tile, first block, end block, ordinal of the segment within its tile}, each lane's segments in the order they
 * run; capacity: M in blocks.  Returns the number of segments. */
long scrappie_hip_decoder_lanes(const int *tile_T, size_t ntile, int ncu, int *nwg, int *capacity, int *lane_off, int *seg, size_t cap);

size_t scrappie_hip_min_samples(scrappie_hip_engine *e, int model);
int scrappie_hip_model_stride(scrappie_hip_engine *e, int model);
void scrappie_hip_set_profiling(scrappie_hip_engine *e, int on);
int scrappie_hip_get_timing(scrappie_hip_engine *e, scrappie_hip_timing *t);
/* upper bound on reads per launch group (default 16384) */
void scrappie_hip_set_max_launch_reads(scrappie_hip_engine *e, size_t n);
/* upper bound on column blocks (16 reads x 1 block) per launch group; 0 (default) = derived from the
 * device's memory (about 70 % of it across the arena).  scrappie_hip_basecall_batch/_device cut their
 * input into launch groups under both bounds and keep two groups in flight. */
void scrappie_hip_set_max_launch_blocks(scrappie_hip_engine *e, size_t n);
/* the cut itself (host only, no device): starts[] takes the first read of each group, input order
 * kept; returns the number of groups (even if > cap), -1 if one read alone exceeds max_blocks */
long scrappie_hip_plan_groups(const uint32_t *lengths, size_t n, int stride, size_t max_reads, size_t max_blocks,
                              size_t *starts, size_t cap);
/* Host threads an engine of this process uses for gathering and stitching: min(CPUs of the affinity mask, the cgroup's
 * cpu.max quota, 32), divided by LOCAL_WORLD_SIZE when a launcher runs one process per GPU (torchrun sets it), or
 * SCRAPPIE_HIP_HOST_THREADS.  Read once per process. */
unsigned scrappie_hip_host_thread_budget(void);
/* ... and without the per-engine cap of 32: the CPUs the process may use (affinity, cgroup quota, / LOCAL_WORLD_SIZE) -- what `scrappie raw` sizes its
 * loader team from: 16 loader threads per GPU (fast5 input needs ~14 to feed one engine, profiles/r6_cli_rate.txt), as many as there are CPUs at most */
unsigned scrappie_hip_host_cpu_budget(void);
/* device memory helpers so a host with no HIP runtime of its own can stage data */
void *scrappie_hip_device_alloc(scrappie_hip_engine *e, size_t nbytes);
void scrappie_hip_device_free(scrappie_hip_engine *e, void *dptr);
int scrappie_hip_memcpy_h2d(scrappie_hip_engine *e, void *dst, const void *src, size_t nbytes);
int scrappie_hip_synchronize(scrappie_hip_engine *e);

/* read_raw (src/fast5_interface.c:130): first read of a fast5 file, optionally
 * scaled to pA; also reads headerless *.f32 / *.i16 signal files.  HDF5 is
 * resolved with dlopen at run time (scrappie_hip_have_hdf5() tells whether one
 * was found).  Caller frees .raw and .uuid; .raw == NULL on failure. */
raw_table scrappie_hip_read_raw(const char *filename, bool scale_to_pA);
/* ... with the samples placed where `alloc` says (NULL, or a NULL return: malloc as above) -- e.g. scrappie_hip_prep_alloc, so
 * that a loader thread reads a file straight into the pinned buffer the device copies from */
typedef float *(*scrappie_hip_sample_alloc)(void *ctx, size_t nsample);
raw_table scrappie_hip_read_raw_into(const char *filename, bool scale_to_pA, scrappie_hip_sample_alloc alloc, void *ctx);
int scrappie_hip_have_hdf5(void);
/* offset, range, digitisation attributes of a fast5 file; 0 on success */
int scrappie_hip_fast5_scaling(const char *filename, float out[3]);

/* FASTA / SAM record exactly as src/scrappie_raw.c:317-331 prints them.
 * Returns the number of characters written (snprintf semantics). */
int scrappie_hip_format_fasta(char *buf, size_t buflen, const char *uuid, const char *readname,
                              bool uuid_primary, const char *prefix, const scrappie_hip_call *res,
                              size_t nsample, size_t trim_start, size_t trim_end);
int scrappie_hip_format_sam(char *buf, size_t buflen, const char *uuid, const char *readname,
                            bool uuid_primary, const char *prefix, const scrappie_hip_call *res);

#ifdef __cplusplus
}
#endif
#endif /* SCRAPPIE_HIP_H */
