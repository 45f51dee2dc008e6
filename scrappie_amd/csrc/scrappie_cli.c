/* scrappie_cli.c -- what the subcommands of `scrappie` share (scrappie_cli.h) */
#define _GNU_SOURCE
#include <libgen.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>

#include "scrappie_cli.h"

int cli_parse_pair(const char *arg, long *n, double *x) {
    const char *colon = strchr(arg, ':');
    *n = strtol(arg, NULL, 10);                             /* (stops at the colon, if not before) */
    *x = colon ? strtod(colon + 1, NULL) : 0.0;
    return colon != NULL;
}

int cli_parse_trim(const char *arg, int *start, int *end) {
    long n;
    double x;
    if (!cli_parse_pair(arg, &n, &x)) x = (double)n;        /* a single number trims both ends (src/scrappie_raw.c:160-166) */
    if (n < 0 || n > INT_MAX || !(x >= 0 && x <= INT_MAX)) return -1;
    *start = (int)n; *end = (int)x;
    return 0;
}

int cli_parse_segmentation(const char *arg, int *chunk, double *pct) {
    long n;
    double x;
    if (!cli_parse_pair(arg, &n, &x)) return -1;
    *chunk = (int)n; *pct = x;
    return 0;
}

FILE *cli_open_output(const char *path) {
    FILE *fh = fopen(path, "w");
    if (!fh) fprintf(stderr, "scrappie: Failed to open \"%s\" for output.\n", path);
    return fh;
}

void cli_licence(void) { puts("Mozilla Public License 2.0 applies to the reference interface this build follows."); exit(EXIT_SUCCESS); }

char *cli_model_path(const char *model, const char *model_file) {
    char *path = NULL;
    const char *dir = getenv("SCRAPPIE_MODEL_DIR");
    if (model_file) path = strdup(model_file);
    else if (dir && asprintf(&path, "%s/%s.scrm", dir, model) < 0) path = NULL;
    if (!path) fprintf(stderr, "scrappie: no weights for model %s (weights are data, not part of this build): give --model-file or set SCRAPPIE_MODEL_DIR\n", model);
    return path;
}

scrappie_hip_engine *cli_open_model(int device, const char *model, const char *model_file, int *handle) {
    scrappie_hip_engine *e = scrappie_hip_engine_create(device);
    if (!e) { fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error()); return NULL; }
    char *path = cli_model_path(model, model_file);
    *handle = path ? scrappie_hip_load_model(e, model, path) : -1;
    if (path && *handle < 0) fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
    free(path);
    if (*handle < 0) { scrappie_hip_engine_destroy(e); return NULL; }
    return e;
}

raw_table cli_prepare_read(raw_table rt, int trim_start, int trim_end, int chunk, float thresh, int normalise) {
    char *uuid = rt.uuid;
    if (rt.raw && chunk > 0) {
        rt = trim_and_segment_raw(rt, (size_t)trim_start, (size_t)trim_end, (size_t)chunk, thresh);      /* (frees the samples of a read it trims away, not its uuid) */
    } else if (rt.raw) {
        rt.start = (rt.n - rt.start) > (size_t)trim_start ? rt.start + (size_t)trim_start : rt.n;
        rt.end = rt.end > (size_t)trim_end ? rt.end - (size_t)trim_end : 0;
        if (rt.start >= rt.end) { free(rt.raw); rt.raw = NULL; }
    }
    if (!rt.raw) { free(uuid); return (raw_table){0}; }
    if (normalise) medmad_normalise_array(rt.raw + rt.start, rt.end - rt.start);
    return rt;
}

raw_table cli_load_read(const char *path, int trim_start, int trim_end, int chunk, float thresh, int normalise) {
    return cli_prepare_read(scrappie_hip_read_raw(path, true), trim_start, trim_end, chunk, thresh, normalise);
}

int cli_read_fasta(const char *path, struct cli_fasta **recs, size_t *nrec, size_t limit) {
    FILE *fh = fopen(path, "r");
    if (!fh) return -1;
    char *line = NULL;
    size_t cap = 0, scap = 0;
    ssize_t got;
    struct cli_fasta *cur = NULL;
    while ((got = getline(&line, &cap, fh)) != -1) {
        while (got > 0 && (line[got - 1] == '\n' || line[got - 1] == '\r')) line[--got] = '\0';
        if (line[0] == '>') {
            if (limit && *nrec >= limit) break;
            struct cli_fasta *grown = realloc(*recs, (*nrec + 1) * sizeof **recs);
            if (!grown) break;
            *recs = grown;
            cur = &grown[(*nrec)++];
            cur->name = strndup(line + 1, strcspn(line + 1, " \t"));
            cur->seq = calloc(1, 1); cur->n = 0; scap = 1;
            continue;
        }
        if (!cur || got == 0 || !cur->seq) continue;
        if (cur->n + (size_t)got + 1 > scap) {
            scap = 2 * (cur->n + (size_t)got + 1);
            char *s = realloc(cur->seq, scap);
            if (!s) break;
            cur->seq = s;
        }
        memcpy(cur->seq + cur->n, line, (size_t)got); cur->n += (size_t)got; cur->seq[cur->n] = '\0';
    }
    free(line);
    fclose(fh);
    return 0;
}

void cli_free_fasta(struct cli_fasta *recs, size_t nrec) {
    for (size_t i = 0; i < nrec; i++) { free(recs[i].name); free(recs[i].seq); }
    free(recs);
}

char *cli_record_name(const char *path, const char *uuid, int uuid_primary) {
    if (uuid_primary) return strdup(uuid ? uuid : "");
    char *copy = strdup(path);                              /* (basename may write to its argument) */
    char *name = copy ? strdup(basename(copy)) : NULL;
    free(copy);
    return name;
}

/* The subcommands (src/scrappie.c:13, scrappie_subcommands.c:6).  The entries are weak, so that this file links with the
 * subcommands that are there (the sanitizer builds of the tests leave most of them out); one that is not says so. */
#define WEAK(f) extern __typeof__(f) f __attribute__((weak))
WEAK(main_raw); WEAK(main_seqmappy); WEAK(main_squiggle); WEAK(main_mappy); WEAK(main_event_table); WEAK(main_events);
static const struct { const char *name; int (*entry)(int, char **); const char *help; } subcommands[] = {
    {"raw", main_raw, "Basecall from raw signal (MI355X)"},
    {"seqmappy", main_seqmappy, "Map reads to sequences (local-global Viterbi on the posterior)"},
    {"squiggle", main_squiggle, "Predict the squiggle of base sequences"},
    {"mappy", main_mappy, "Map a read's signal to the squiggle predicted for a sequence"},
    {"event_table", main_event_table, "Detect events and print the event table of each read"},
    {"events", main_events, "Basecall via events, with the dwell correction of homopolymer lengths"},
};
#define NSUB (sizeof subcommands / sizeof subcommands[0])

int cli_main(int argc, char **argv) {
    if (argc < 2 || 0 == strcmp(argv[1], "help") || 0 == strcmp(argv[1], "--help")) {
        puts("Usage: scrappie <subcommand> [options]");
        for (size_t i = 0; i < NSUB; i++) printf("  %-9s  %s\n", subcommands[i].name, subcommands[i].help);
        printf("  %-9s  %s\n", "version", "Print version");
        return argc < 2 ? EXIT_FAILURE : EXIT_SUCCESS;
    }
    if (0 == strcmp(argv[1], "version") || 0 == strcmp(argv[1], "--version")) { puts("scrappie (MI355X hot-path build) 0.1.0, interface of scrappie 1.4"); return EXIT_SUCCESS; }
    for (size_t i = 0; i < NSUB; i++)
        if (0 == strcmp(argv[1], subcommands[i].name) && subcommands[i].entry) return subcommands[i].entry(argc - 1, argv + 1);
    fprintf(stderr, "scrappie: subcommand \"%s\" is not part of this build (only", argv[1]);
    for (size_t i = 0; i < NSUB; i++) fprintf(stderr, "%s `%s`", i == 0 ? "" : i + 1 < NSUB ? "," : " and", subcommands[i].name);
    fputs(")\n", stderr);
    return EXIT_FAILURE;
}
