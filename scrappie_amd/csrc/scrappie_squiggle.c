/* scrappie_squiggle.c -- the `scrappie squiggle` and `scrappie mappy` command lines over libscrappie_hip.so
 * (src/scrappie_squiggle.c, src/scrappie_mappy.c).
 *
 * Same options, defaults and output as the reference's subcommands.  squiggle: the predicted squiggle of every record of
 * every FASTA file, all of them in ONE scrappie_hip_squiggle_predict_batch call, written in input order; a record the
 * network refuses (a base outside ACGT, fewer bases than the window needs) is skipped, as the reference skips a NULL
 * squiggle.  mappy: the first record's squiggle, then squiggle_match_viterbi of the read against it.  Added: --model-file /
 * --device as `scrappie raw` takes them (the weights are data: default $SCRAPPIE_MODEL_DIR/<model>.scrm); mappy --band N, the
 * match inside the diagonal band of half-width N positions (scrappie_hip_squiggle_diagonal_band).
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scrappie_cli.h"

static int squiggle_model_ok(const char *name) {      /* scrappie_stdlib.h: get_squiggle_model */
    return !strcmp(name, "squiggle_r94") || !strcmp(name, "squiggle_r94_rna") || !strcmp(name, "squiggle_r10");
}

static void squiggle_usage(FILE *fh) {
    fputs("Usage: scrappie squiggle [OPTION...] fasta [fasta ...]\n"
          "Scrappie squiggler\n\n"
          "  -l, --limit=nreads         Maximum number of reads to call (0 is unlimited)\n"
          "  -m, --model=name           Squiggle model to use: \"squiggle_r94\", \"squiggle_r94_rna\", \"squiggle_r10\"\n"
          "  -o, --output=filename      Write to file rather than stdout\n"
          "  -p, --prefix=string        Prefix to append to name of each read\n"
          "      --rescale, --no-rescale   Rescale network output (default) or don't\n"
          "      --licence, --license   Print licensing information\n"
          "      --model-file=path      Weight container (.scrm); default $SCRAPPIE_MODEL_DIR/<model>.scrm\n"
          "      --device=N             GPU to run on (default 0)\n"
          "All records of all files are predicted in one batched engine call and written in input order.\n", fh);
}

int main_squiggle(int argc, char **argv) {
    enum { O_RESCALE = 256, O_NORESCALE, O_LIC, O_MFILE, O_DEV };
    static const struct option lo[] = {
        {"model", 1, 0, 'm'}, {"limit", 1, 0, 'l'}, {"output", 1, 0, 'o'}, {"prefix", 1, 0, 'p'}, {"rescale", 0, 0, O_RESCALE},
        {"no-rescale", 0, 0, O_NORESCALE}, {"licence", 0, 0, O_LIC}, {"license", 0, 0, O_LIC}, {"model-file", 1, 0, O_MFILE},
        {"device", 1, 0, O_DEV}, {"help", 0, 0, '?'}, {0, 0, 0, 0}};
    /* defaults: scrappie_squiggle.c:47-54 */
    const char *model = "squiggle_r94", *model_file = NULL;
    FILE *out = stdout;
    int limit = 0, rescale = 1, device = 0, h, c;
    optind = 1;
    while ((c = getopt_long(argc, argv, "m:l:o:p:", lo, NULL)) != -1) {
        switch (c) {
        case 'm':
            if (!squiggle_model_ok(optarg)) { fprintf(stderr, "scrappie: Invalid squiggle model name \"%s\"\n", optarg); return EXIT_FAILURE; }
            model = optarg;
            break;
        case 'l':
            limit = atoi(optarg);
            if (limit < 0) { fprintf(stderr, "scrappie: --limit wants a count\n"); return EXIT_FAILURE; }
            break;
        case 'o': if (!(out = cli_open_output(optarg))) return EXIT_FAILURE; break;
        case 'p': break;                 /* accepted; the reference's squiggle never prints it */
        case O_RESCALE: rescale = 1; break;
        case O_NORESCALE: rescale = 0; break;
        case O_LIC: cli_licence(); break;
        case O_MFILE: model_file = optarg; break;
        case O_DEV: device = atoi(optarg); break;
        default: squiggle_usage(stderr); return EXIT_FAILURE;
        }
    }
    if (argc - optind <= 0) { squiggle_usage(stderr); return EXIT_FAILURE; }
    char *mpath = cli_model_path(model, model_file);      /* (the weights first, then the engine) */
    scrappie_hip_engine *e = mpath ? cli_open_model(device, model, mpath, &h) : NULL;
    free(mpath);
    if (!e) return EXIT_FAILURE;

    struct cli_fasta *recs = NULL;
    size_t nrec = 0;
    for (int fn = optind; fn < argc; fn++) {
        if (limit > 0 && nrec >= (size_t)limit) break;
        if (cli_read_fasta(argv[fn], &recs, &nrec, (size_t)limit)) fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n\n", argv[fn]);
    }
    int rc = EXIT_SUCCESS;
    int **codes = calloc(nrec ? nrec : 1, sizeof *codes);
    size_t *lens = calloc(nrec ? nrec : 1, sizeof *lens);
    scrappie_matrix *sq = calloc(nrec ? nrec : 1, sizeof *sq);
    for (size_t i = 0; i < nrec; i++) {
        codes[i] = recs[i].seq ? encode_bases_to_integers(recs[i].seq, recs[i].n, 1) : NULL;      /* NULL: refused below, like a NULL sequence */
        lens[i] = recs[i].n;
    }
    if (scrappie_hip_squiggle_predict_batch(e, model, (const int *const *)codes, lens, nrec, rescale, sq) != 0) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        for (size_t i = 0; i < nrec; i++) {
            if (!sq[i]) continue;
            /* scrappie_squiggle.c:157-164 */
            fprintf(out, "#%s\n", recs[i].name ? recs[i].name : "");
            fprintf(out, "pos\tbase\tcurrent\tsd\tdwell\n");
            for (size_t k = 0; k < sq[i]->nc; k++) {
                const float *col = sq[i]->data.f + k * sq[i]->stride;
                fprintf(out, "%zu\t%c\t%3.6f\t%3.6f\t%3.6f\n", k, recs[i].seq[k], col[0], col[1], col[2]);
            }
        }
    }
    for (size_t i = 0; i < nrec; i++) { free(codes[i]); free_scrappie_matrix(sq[i]); }
    free(codes); free(lens); free(sq);
    cli_free_fasta(recs, nrec);
    if (out != stdout) fclose(out);
    scrappie_hip_engine_destroy(e);
    return rc;
}

static void mappy_usage(FILE *fh) {
    fputs("Usage: scrappie mappy [OPTION...] fasta fast5\n"
          "Scrappie squiggler\n\n"
          "  -b, --backprob=probability Probability of backwards movement\n"
          "  -k, --skippen=float        Penalty for skipping position\n"
          "  -l, --localpen=float       Penalty for local matching\n"
          "  -m, --minscore=float       Minimum possible score for matching emission\n"
          "      --model=name           Squiggle model to use: \"squiggle_r94\", \"squiggle_r94_rna\" or \"squiggle_r10\"\n"
          "  -o, --output=filename      Write to file rather than stdout\n"
          "  -p, --prefix=string        Prefix to append to name of read\n"
          "  -r, --rate=float           Translocation rate of read relative to standard squiggle\n"
          "  -s, --segmentation=chunk:percentile\n"
          "                             Chunk size and percentile for variance based segmentation\n"
          "  -t, --trim=start:end       Number of samples to trim, as start:end\n"
          "      --licence, --license   Print licensing information\n"
          "      --model-file=path      Weight container (.scrm); default $SCRAPPIE_MODEL_DIR/<model>.scrm\n"
          "      --device=N             GPU to run on (default 0)\n"
          "      --band=N               Map inside the diagonal band of half-width N positions (default: no band)\n"
          "      --all-records          Match the read against every record of the fasta: a table of their scores, then the best\n"
          "                             record's mapping (not with --band)\n"
          "      --inside               The read lies somewhere INSIDE the (longer) sequence: entering and leaving it is free at every\n"
          "                             position; the header gains `positions first..last` (the path lies in [first, last) of the\n"
          "                             sequence) (not with --band or --all-records)\n", fh);
}

/* scrappie_mappy.c:215-228: the header line and one line per sample of the read */
static void mappy_print(FILE *out, const char *fast5, const char *fasta, float score, const raw_table *rt, const int32_t *path, const_scrappie_matrix sq,
                        const char *seq, const size_t *span) {
    if (span) fprintf(out, "# %s to %s  (score = %f, positions %zu..%zu)\n", fast5, fasta, score, span[0], span[1]);      /* --inside */
    else fprintf(out, "# %s to %s  (score = %f)\n", fast5, fasta, score);
    fprintf(out, "idx\tsignal\tpos\tbase\tcurrent\tsd\tdwell\n");
    for (size_t i = 0; i < rt->n; i++) {
        const int32_t pos = path[i];
        if (pos >= 0) {
            const float *col = sq->data.f + (size_t)pos * sq->stride;
            fprintf(out, "%zu\t%3.6f\t%d\t%c\t%3.6f\t%3.6f\t%3.6f\n", i, rt->raw[i], pos, seq[pos], col[0], expf(col[1]), expf(-col[2]));
        } else {
            fprintf(out, "%zu\t%3.6f\t%d\tN\tnan\tnan\tnan\n", i, (i >= rt->start && i < rt->end) ? rt->raw[i] : NAN, pos);
        }
    }
}

/* --all-records: the read against every record of the fasta in one pass (scrappie_hip_squiggle_match_multi_batch): one batched
 * prediction, the records' scores as a table, then the best record as plain mappy prints it */
static int mappy_all_records(scrappie_hip_engine *e, const char *model, const char *fasta, const char *fast5, const raw_table *rt,
                             const scrappie_hip_squiggle_params *p, FILE *out) {
    struct cli_fasta *recs = NULL;
    size_t nrec = 0;
    if (cli_read_fasta(fasta, &recs, &nrec, 0) || nrec == 0) {
        fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n\n", fasta);
        cli_free_fasta(recs, nrec);
        return EXIT_FAILURE;
    }
    int rc = EXIT_FAILURE;
    int **codes = calloc(nrec, sizeof *codes);
    size_t *lens = calloc(nrec, sizeof *lens);
    scrappie_matrix *sq = calloc(nrec, sizeof *sq);
    scrappie_hip_squiggle_target *tg = calloc(nrec, sizeof *tg);
    scrappie_hip_squiggle_multi_result res = {0};
    if (!codes || !lens || !sq || !tg) { fprintf(stderr, "scrappie: out of memory\n"); goto done; }
    for (size_t k = 0; k < nrec; k++) {          /* a record that cannot be encoded is predicted as an empty sequence: refused, scored nan */
        codes[k] = recs[k].seq && recs[k].n ? encode_bases_to_integers(recs[k].seq, recs[k].n, 1) : NULL;
        lens[k] = codes[k] ? recs[k].n : 0;
    }
    if (scrappie_hip_squiggle_predict_batch(e, model, (const int *const *)codes, lens, nrec, 0, sq) != 0) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        goto done;
    }
    for (size_t k = 0; k < nrec; k++)
        if (sq[k]) { tg[k].params = sq[k]->data.f; tg[k].npos = sq[k]->nc; tg[k].stride = sq[k]->stride; }
    const scrappie_hip_squiggle_candidates cd = {tg, nrec};
    if (scrappie_hip_squiggle_match_multi_batch(e, rt, &cd, 1, p, 1, 1, &res) != 0 || !res.score) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        goto done;
    }
    const size_t ns = rt->end > rt->start ? rt->end - rt->start : 1;
    fprintf(out, "record\tname\tscore\tper_sample\n");
    for (size_t k = 0; k < nrec; k++) fprintf(out, "%zu\t%s\t%f\t%f\n", k, recs[k].name ? recs[k].name : "", res.score[k], res.score[k] / (float)ns);
    if (res.best < 0 || !res.path) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        goto done;
    }
    mappy_print(out, fast5, fasta, res.score[res.best], rt, res.path, sq[res.best], recs[res.best].seq, NULL);
    rc = EXIT_SUCCESS;
done:
    scrappie_hip_free_squiggle_multi_results(&res, 1);
    for (size_t k = 0; k < nrec; k++) { if (codes) free(codes[k]); if (sq) free_scrappie_matrix(sq[k]); }
    free(codes); free(lens); free(sq); free(tg);
    cli_free_fasta(recs, nrec);
    return rc;
}

int main_mappy(int argc, char **argv) {
    enum { O_MODEL = 256, O_LIC, O_MFILE, O_DEV, O_BAND, O_ALL, O_INSIDE };
    static const struct option lo[] = {
        {"all-records", 0, 0, O_ALL}, {"inside", 0, 0, O_INSIDE}, {"band", 1, 0, O_BAND}, {"model", 1, 0, O_MODEL}, {"backprob", 1, 0, 'b'}, {"skippen", 1, 0, 'k'}, {"localpen", 1, 0, 'l'}, {"minscore", 1, 0, 'm'},
        {"output", 1, 0, 'o'}, {"prefix", 1, 0, 'p'}, {"rate", 1, 0, 'r'}, {"segmentation", 1, 0, 's'}, {"trim", 1, 0, 't'},
        {"licence", 0, 0, O_LIC}, {"license", 0, 0, O_LIC}, {"model-file", 1, 0, O_MFILE}, {"device", 1, 0, O_DEV}, {"help", 0, 0, '?'},
        {0, 0, 0, 0}};
    /* defaults: scrappie_mappy.c:59-75 */
    scrappie_hip_squiggle_params p = scrappie_hip_default_squiggle_params();
    const char *model = "squiggle_r94", *model_file = NULL;
    FILE *out = stdout;
    int trim_start = 200, trim_end = 10, varseg_chunk = 100, device = 0, h, c;
    long band = -1;                      /* half-width of the diagonal band in positions; < 0: none */
    int all_records = 0, inside = 0;
    float varseg_thresh = 0.0f;
    double pct;
    optind = 1;
    while ((c = getopt_long(argc, argv, "b:k:l:m:o:p:r:s:t:", lo, NULL)) != -1) {
        switch (c) {
        case O_MODEL:
            if (!squiggle_model_ok(optarg)) { fprintf(stderr, "scrappie: Invalid squiggle model name \"%s\"\n", optarg); return EXIT_FAILURE; }
            model = optarg;
            break;
        case 'b':
            p.prob_back = (float)atof(optarg);
            if (!(p.prob_back >= 0.0f && p.prob_back < 1.0f)) { fprintf(stderr, "scrappie: Backwards probability must be in [0, 1). Got %f\n", p.prob_back); return EXIT_FAILURE; }
            break;
        case 'k': p.skip_pen = (float)atof(optarg); break;
        case 'l': p.local_pen = (float)atof(optarg); break;
        case 'm': p.minscore = (float)atof(optarg); break;
        case 'o': if (!(out = cli_open_output(optarg))) return EXIT_FAILURE; break;
        case 'p': break;                 /* accepted; the reference's mappy never prints it */
        case 'r':
            p.rate = (float)atof(optarg);
            if (!(p.rate > 0.0f)) { fprintf(stderr, "scrappie: Rate must be positive, got %f\n", p.rate); return EXIT_FAILURE; }
            break;
        case 's':
            varseg_thresh = cli_parse_segmentation(optarg, &varseg_chunk, &pct) ? -1.0f : (float)(pct / 100.0);       /* (no colon: refused like a percentile out of range) */
            if (varseg_chunk < 0 || !(varseg_thresh > 0.0f && varseg_thresh < 1.0f)) { fprintf(stderr, "scrappie: --segmentation should be of form chunk:percentile\n"); return EXIT_FAILURE; }
            break;
        case 't': if (cli_parse_trim(optarg, &trim_start, &trim_end)) { fprintf(stderr, "scrappie: --trim wants start:end\n"); return EXIT_FAILURE; } break;
        case O_LIC: cli_licence(); break;
        case O_MFILE: model_file = optarg; break;
        case O_DEV: device = atoi(optarg); break;
        case O_ALL: all_records = 1; break;
        case O_INSIDE: inside = 1; break;
        case O_BAND:
            band = atol(optarg);
            if (band < 0) { fprintf(stderr, "scrappie: --band wants a half-width in positions, 0 or more\n"); return EXIT_FAILURE; }
            break;
        default: mappy_usage(stderr); return EXIT_FAILURE;
        }
    }
    if (argc - optind <= 0) { mappy_usage(stderr); return EXIT_FAILURE; }
    if (argc - optind < 2) { fprintf(stderr, "scrappie: fast5 file is a required argument\n"); return EXIT_FAILURE; }      /* scrappie_mappy.c:152 */
    if (all_records && band >= 0) { fprintf(stderr, "scrappie: --all-records maps without a band; it cannot be combined with --band\n"); return EXIT_FAILURE; }
    if (inside && (all_records || band >= 0)) { fprintf(stderr, "scrappie: --inside maps without a band into one sequence; it cannot be combined with --band or --all-records\n"); return EXIT_FAILURE; }
    const char *fasta = argv[optind], *fast5 = argv[optind + 1];
    char *mpath = cli_model_path(model, model_file);      /* (the weights first, then the engine) */
    scrappie_hip_engine *e = mpath ? cli_open_model(device, model, mpath, &h) : NULL;
    free(mpath);
    if (!e) return EXIT_FAILURE;
    if (all_records) {
        raw_table art = cli_load_read(fast5, trim_start, trim_end, varseg_chunk, varseg_thresh, 1);
        int arc = EXIT_FAILURE;
        if (!art.raw) fprintf(stderr, "scrappie: Failed to open \"%s\" for input and trim signal.\n\n", fast5);
        else arc = mappy_all_records(e, model, fasta, fast5, &art, &p, out);
        free(art.raw); free(art.uuid);
        if (out != stdout) fclose(out);
        scrappie_hip_engine_destroy(e);
        return arc;
    }

    int rc = EXIT_FAILURE;
    struct cli_fasta *recs = NULL;
    size_t nrec = 0;
    raw_table rt = {0};
    int *codes = NULL;
    scrappie_matrix sq = NULL;
    scrappie_hip_squiggle_result res = {0};
    scrappie_hip_squiggle_local_result lres = {0};
    int32_t *low = NULL;
    if (cli_read_fasta(fasta, &recs, &nrec, 1) || nrec == 0 || !recs[0].seq || recs[0].n == 0) {
        fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n\n", fasta);
        goto done;
    }
    /* scrappie_mappy.c:197-204 */
    rt = cli_load_read(fast5, trim_start, trim_end, varseg_chunk, varseg_thresh, 1);
    if (!rt.raw) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input and trim signal.\n\n", fast5); goto done; }

    rc = EXIT_SUCCESS;                   /* from here on the reference prints what it has and succeeds */
    codes = encode_bases_to_integers(recs[0].seq, recs[0].n, 1);
    const int *cp = codes;
    if (!codes || scrappie_hip_squiggle_predict_batch(e, model, &cp, &recs[0].n, 1, 0, &sq) != 0 || !sq) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        goto done;
    }
    scrappie_hip_squiggle_target tg = {sq->data.f, sq->nc, sq->stride};
    if (inside) {                        /* the read somewhere inside the sequence (scrappie_hip_squiggle_match_local_batch) */
        if (scrappie_hip_squiggle_match_local_batch(e, &rt, &tg, 1, &p, 1, 1, &lres) != 0 || !lres.path) {
            fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
            rc = EXIT_FAILURE;
            goto done;
        }
        const size_t span[2] = {lres.first, lres.last};
        mappy_print(out, fast5, fasta, lres.score, &rt, lres.path, sq, recs[0].seq, span);
        goto done;
    }
    scrappie_hip_squiggle_band bd = {NULL, 0};
    if (band >= 0 && rt.end > rt.start) {
        low = malloc((rt.end - rt.start) * sizeof *low);
        if (!low) { fprintf(stderr, "scrappie: out of memory\n"); rc = EXIT_FAILURE; goto done; }
        bd.low = low;
        bd.width = scrappie_hip_squiggle_diagonal_band(rt.end - rt.start, sq->nc, (size_t)band, low);
    }
    if (scrappie_hip_squiggle_match_banded_batch(e, &rt, &tg, &bd, 1, &p, 1, 1, &res) != 0 || !res.path) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
        goto done;
    }
    mappy_print(out, fast5, fasta, res.score, &rt, res.path, sq, recs[0].seq, NULL);
done:
    scrappie_hip_free_squiggle_results(&res, 1);
    scrappie_hip_free_squiggle_local_results(&lres, 1);
    free_scrappie_matrix(sq);
    free(codes);
    free(low);
    free(rt.raw); free(rt.uuid);
    cli_free_fasta(recs, nrec);
    if (out != stdout) fclose(out);
    scrappie_hip_engine_destroy(e);
    return rc;
}
