/* include/pyscrap_events.h -- the cdef line for event detection as scrappy binds it (python/pyscrap.h:65), with the reference's name
 * and signature: appended to the cdef text of include/pyscrap_raw.h it routes scrappy's event-detection helper to this library
 * (`detector_param` is in the struct block build.py already has).  A read without a peak gives .event == NULL. */

event_table detect_events(raw_table const rt, detector_param const edparam);

/* src/decode.h:16-19: the dwell correction `scrappie events` ends with, host C like overlapper.  `dwell_model` is not among the types
 * build.py declares: give cffi `typedef struct { float scale; float base_adj[4]; } dwell_model;` with them. */
char *homopolymer_dwell_correction(const event_table et, const int *seq, size_t nstate, size_t basecall_len);
char *dwell_corrected_overlapper(const int *seq, const int *dwell, int n, int nkmer, const dwell_model dm);
