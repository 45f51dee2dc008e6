/* scrappie_seqmappy.c -- the `scrappie seqmappy` command line over libscrappie_hip.so (src/scrappie_seqmappy.c).
 *
 * Same options, defaults and output as the reference's subcommand: a read's posterior (rgrgr_r94 by default) mapped by
 * local-global Viterbi to the first sequence of a FASTA file, one `block\tpos` line per block.  Added: --model /
 * --model-file / --device as `scrappie raw` takes them, and more `fasta fast5` pairs after the first -- every pair is
 * mapped in ONE scrappie_hip_map_batch call (network, S1 and the mapping on the GPU; only scores and paths return) and
 * the records are written in argument order.  One pair prints exactly what the reference prints.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>

#include "scrappie_hip.h"

int main_seqmappy(int argc, char **argv);

static int parse_pair(const char *arg, long *a, double *b_or_null, long *b_long) {
    /* "start:end" / "chunk:percentile" */
    char *end = NULL;
    *a = strtol(arg, &end, 10);
    if (!end || *end != ':') return -1;
    if (b_long) *b_long = strtol(end + 1, NULL, 10);
    if (b_or_null) *b_or_null = strtod(end + 1, NULL);
    return 0;
}

/* the first record of a FASTA file, its sequence lines joined (NULL if there is none) */
static char *read_fasta_first(const char *path, size_t *n) {
    FILE *fh = fopen(path, "r");
    if (!fh) return NULL;
    char *line = NULL, *seq = NULL;
    size_t cap = 0, len = 0, scap = 0;
    ssize_t got;
    int in_rec = 0;
    while ((got = getline(&line, &cap, fh)) != -1) {
        while (got > 0 && (line[got - 1] == '\n' || line[got - 1] == '\r')) line[--got] = '\0';
        if (line[0] == '>') { if (in_rec) break; in_rec = 1; continue; }
        if (!in_rec || got == 0) continue;
        if (len + (size_t)got + 1 > scap) { scap = 2 * (len + (size_t)got + 1); seq = realloc(seq, scap); if (!seq) break; }
        memcpy(seq + len, line, (size_t)got); len += (size_t)got; seq[len] = '\0';
    }
    free(line);
    fclose(fh);
    if (!in_rec || !seq) { free(seq); return NULL; }
    *n = len;
    return seq;
}

static void seqmappy_usage(FILE *fh) {
    fputs("Usage: scrappie seqmappy [OPTION...] fasta fast5 [fasta fast5 ...]\n"
          "Scrappie seqmappy (local-global)\n\n"
          "  -l, --localpen=float       Penalty for local matching\n"
          "  -m, --min_prob=probability Minimum bound on probability of match\n"
          "  -o, --output=filename      Write to file rather than stdout\n"
          "  -p, --prefix=string        Prefix to append to name of read\n"
          "      --segmentation=chunk:percentile\n"
          "                             Chunk size and percentile for variance based segmentation\n"
          "  -s, --skip=penalty         Penalty for skipping a base\n"
          "  -y, --stay=penalty         Penalty for staying\n"
          "  -t, --trim=start:end       Number of samples to trim, as start:end\n"
          "      --temperature1=factor  Temperature for softmax weights\n"
          "      --temperature2=factor  Temperature for softmax bias\n"
          "      --licence, --license   Print licensing information\n"
          "      --model=name           Raw model to use (default rgrgr_r94)\n"
          "      --model-file=path      Weight container (.scrm); default $SCRAPPIE_MODEL_DIR/<model>.scrm\n"
          "      --device=N             GPU to run on (default 0)\n"
          "Every (fasta, fast5) pair is mapped in one batched engine call; records are written in argument order.\n", fh);
}

int main_seqmappy(int argc, char **argv) {
    enum { O_SEG = 256, O_T1, O_T2, O_LIC, O_MODEL, O_MFILE, O_DEV };
    static const struct option lo[] = {
        {"localpen", 1, 0, 'l'}, {"min_prob", 1, 0, 'm'}, {"output", 1, 0, 'o'}, {"prefix", 1, 0, 'p'},
        {"segmentation", 1, 0, O_SEG}, {"skip", 1, 0, 's'}, {"stay", 1, 0, 'y'}, {"trim", 1, 0, 't'},
        {"temperature1", 1, 0, O_T1}, {"temperature2", 1, 0, O_T2}, {"licence", 0, 0, O_LIC}, {"license", 0, 0, O_LIC},
        {"model", 1, 0, O_MODEL}, {"model-file", 1, 0, O_MFILE}, {"device", 1, 0, O_DEV}, {"help", 0, 0, '?'}, {0, 0, 0, 0}};
    /* defaults: scrappie_seqmappy.c:62-78 */
    scrappie_hip_params p = scrappie_hip_default_params();
    p.local_pen = 4.0f; p.min_prob = 1e-5f; p.stay_pen = 0.0f; p.skip_pen = 0.0f; p.tempW = 1.0f; p.tempb = 1.0f;
    FILE *out = stdout;
    int trim_start = 200, trim_end = 10, varseg_chunk = 100, device = 0;
    float varseg_thresh = 0.0f;
    const char *model = "rgrgr_r94", *model_file = NULL;
    long a, bl;
    double bd;
    int c;
    optind = 1;
    while ((c = getopt_long(argc, argv, "l:m:o:p:s:y:t:", lo, NULL)) != -1) {
        switch (c) {
        case 'l': p.local_pen = (float)atof(optarg); break;
        case 'm': p.min_prob = (float)atof(optarg); break;
        case 'o':
            out = fopen(optarg, "w");
            if (!out) { fprintf(stderr, "scrappie: Failed to open \"%s\" for output.\n", optarg); return EXIT_FAILURE; }
            break;
        case 'p': break;                 /* accepted; the reference's seqmappy never prints it */
        case 's': p.skip_pen = (float)atof(optarg); break;
        case 'y': p.stay_pen = (float)atof(optarg); break;
        case 't':
            if (parse_pair(optarg, &a, NULL, &bl)) bl = a;
            if (a < 0 || bl < 0) { fprintf(stderr, "scrappie: --trim wants start:end\n"); return EXIT_FAILURE; }
            trim_start = (int)a; trim_end = (int)bl;
            break;
        case O_SEG:
            if (parse_pair(optarg, &a, &bd, NULL) || a < 0 || bd <= 0 || bd >= 100) { fprintf(stderr, "scrappie: --segmentation should be of form chunk:percentile\n"); return EXIT_FAILURE; }
            varseg_chunk = (int)a; varseg_thresh = (float)(bd / 100.0);
            break;
        case O_T1: p.tempW = (float)atof(optarg); break;
        case O_T2: p.tempb = (float)atof(optarg); break;
        case O_LIC: puts("Mozilla Public License 2.0 applies to the reference interface this build follows."); exit(EXIT_SUCCESS);
        case O_MODEL:
            if (get_raw_model(optarg) == SCRAPPIE_MODEL_INVALID) { fprintf(stderr, "scrappie: Invalid model name \"%s\"\n", optarg); return EXIT_FAILURE; }
            model = optarg;
            break;
        case O_MFILE: model_file = optarg; break;
        case O_DEV: device = atoi(optarg); break;
        default: seqmappy_usage(stderr); return EXIT_FAILURE;
        }
    }
    const int nargs = argc - optind;
    if (nargs <= 0) { seqmappy_usage(stderr); return EXIT_FAILURE; }
    if (nargs % 2) { fprintf(stderr, "scrappie: fast5 file is a required argument\n"); return EXIT_FAILURE; }    /* scrappie_seqmappy.c:153 */
    const size_t npair = (size_t)nargs / 2;
    char **fasta = argv + optind;        /* fasta[2 i], fast5 = fasta[2 i + 1] */

    scrappie_hip_engine *e = scrappie_hip_engine_create(device);
    if (!e) { fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error()); return EXIT_FAILURE; }
    char *mpath = NULL;
    if (model_file) mpath = strdup(model_file);
    else if (getenv("SCRAPPIE_MODEL_DIR")) { if (asprintf(&mpath, "%s/%s.scrm", getenv("SCRAPPIE_MODEL_DIR"), model) < 0) mpath = NULL; }
    if (!mpath) { fprintf(stderr, "scrappie: no weights for model %s: give --model-file or set SCRAPPIE_MODEL_DIR\n", model); return EXIT_FAILURE; }
    const int h = scrappie_hip_load_model(e, model, mpath);
    free(mpath);
    if (h < 0) { fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error()); return EXIT_FAILURE; }
    int nstate = scrappie_hip_model_states(e, h), klen = 0;
    for (int nk = nstate - 1; nk > 1 && nk % 4 == 0; nk /= 4) klen++;

    raw_table *rts = calloc(npair, sizeof *rts);
    scrappie_hip_map_target *tg = calloc(npair, sizeof *tg);
    scrappie_hip_map_result *res = calloc(npair, sizeof *res);
    int **codes = calloc(npair, sizeof *codes);
    int rc = EXIT_SUCCESS;
    for (size_t i = 0; i < npair; i++) {
        const char *fa = fasta[2 * i], *f5 = fasta[2 * i + 1];
        size_t n = 0;
        char *seq = read_fasta_first(fa, &n);
        if (!seq) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n", fa); rc = EXIT_FAILURE; continue; }
        codes[i] = encode_bases_to_integers(seq, n, (size_t)klen);
        free(seq);
        if (!codes[i]) { fprintf(stderr, "scrappie: cannot encode the sequence of \"%s\": %s\n", fa, scrappie_hip_last_error()); rc = EXIT_FAILURE; continue; }
        tg[i].seq = codes[i]; tg[i].seqlen = n - (size_t)klen + 1;
        /* scrappie_seqmappy.c:187-194 */
        raw_table rt = scrappie_hip_read_raw(f5, true);
        rt = trim_and_segment_raw(rt, (size_t)trim_start, (size_t)trim_end, (size_t)varseg_chunk, varseg_thresh);
        if (!rt.raw) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input and trim signal.\n", f5); rc = EXIT_FAILURE; continue; }
        medmad_normalise_array(rt.raw + rt.start, rt.end - rt.start);
        rts[i] = rt;
    }
    if (scrappie_hip_map_batch(e, h, rts, tg, npair, &p, 1, 1, res) != 0) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        for (size_t i = 0; i < npair; i++) {
            if (!rts[i].raw || !codes[i]) continue;
            if (!res[i].path) { fprintf(stderr, "scrappie: Failed to map \"%s\" to \"%s\"\n", fasta[2 * i + 1], fasta[2 * i]); rc = EXIT_FAILURE; continue; }
            const float score = res[i].score;
            const size_t nblock = res[i].nblock;
            fprintf(out, "# %s to %s -- score %f over %zu blocks (%f per block)\n", fasta[2 * i + 1], fasta[2 * i], -score, nblock, -score / nblock);
            fprintf(out, "block\tpos\n");
            for (size_t b = 0; b < nblock; b++) fprintf(out, "%zu\t%d\n", b, res[i].path[b]);
        }
    }
    scrappie_hip_free_map_results(res, npair);
    for (size_t i = 0; i < npair; i++) { free(codes[i]); free(rts[i].raw); free(rts[i].uuid); }
    free(codes); free(res); free(tg); free(rts);
    if (out != stdout) fclose(out);
    scrappie_hip_engine_destroy(e);
    return rc;
}
