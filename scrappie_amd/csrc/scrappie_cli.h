/* scrappie_cli.h -- what the subcommands of `scrappie` share: option grammar, weights, reading and preparing a read, FASTA input,
 * record names and the dispatch.  Host C over the public C ABI (scrappie_hip.h); linked into the command line alone. */
#ifndef SCRAPPIE_CLI_H
#define SCRAPPIE_CLI_H
#include <stdio.h>
#include "scrappie_hip.h"

/* "N[:X]": *n = the leading decimal integer of the text before the first colon, *x = the number after it (0 without one), as atoi /
 * atof read them (src/scrappie_raw.c:159-191).  Returns whether there is a colon. */
int cli_parse_pair(const char *arg, long *n, double *x);
/* --trim N[:M]; a missing :M means M = N.  -1 (nothing written) if either is negative */
int cli_parse_trim(const char *arg, int *start, int *end);
/* --segmentation chunk:percentile, *pct as given (0..100).  -1 without a colon; the ranges are the subcommand's to check */
int cli_parse_segmentation(const char *arg, int *chunk, double *pct);
/* -o: the file opened for writing, or NULL with the message on stderr */
FILE *cli_open_output(const char *path);
/* --licence: prints it and exits */
void cli_licence(void);
/* where the weights of `model` are: model_file if given, else $SCRAPPIE_MODEL_DIR/<model>.scrm; malloc'd, or NULL with the message on stderr */
char *cli_model_path(const char *model, const char *model_file);
/* an engine on `device` with `model` loaded from cli_model_path(model, model_file), its handle in *handle; NULL with the reason on stderr.
 * The engine comes first; a subcommand that looks for the weights first calls cli_model_path itself and passes what it returns. */
scrappie_hip_engine *cli_open_model(int device, const char *model, const char *model_file, int *handle);
/* a read that has been read, prepared (src/scrappie_raw.c:271-277): trim_and_segment_raw, or with chunk 0 the fixed trims alone (src/scrappie_common.c:14-20);
 * then, if asked, medmad_normalise_array on the window.  A read of which nothing is left comes back zeroed, its samples and uuid freed. */
raw_table cli_prepare_read(raw_table rt, int trim_start, int trim_end, int chunk, float thresh, int normalise);
/* scrappie_hip_read_raw(path, true), then cli_prepare_read */
raw_table cli_load_read(const char *path, int trim_start, int trim_end, int chunk, float thresh, int normalise);
/* the records of a FASTA file appended to *recs (at most `limit` in all, 0: no limit): the name is the header up to the first
 * blank, the sequence its lines joined; -1 if the file cannot be opened */
struct cli_fasta { char *name, *seq; size_t n; };
int cli_read_fasta(const char *path, struct cli_fasta **recs, size_t *nrec, size_t limit);
void cli_free_fasta(struct cli_fasta *recs, size_t nrec);
/* the name a record goes by: the read's uuid if uuid_primary, else the file's basename; malloc'd */
char *cli_record_name(const char *path, const char *uuid, int uuid_primary);
/* `scrappie <subcommand> ...`: help, version and the subcommands, which are these */
int cli_main(int argc, char **argv);
int main_raw(int argc, char **argv), main_seqmappy(int argc, char **argv), main_squiggle(int argc, char **argv), main_mappy(int argc, char **argv),
    main_event_table(int argc, char **argv), main_events(int argc, char **argv);
#endif
