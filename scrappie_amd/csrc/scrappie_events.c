/* scrappie_events.c -- the `scrappie events` command line over libscrappie_hip.so (src/scrappie_events.c).
 *
 * The reference's options, defaults and output: every file is read in pA (read_raw(file, true)), trimmed and segmented
 * (trim_and_segment_raw: --trim 200:10, --segmentation 100:0), its events are detected, called with the events model and stitched,
 * with the dwell correction of homopolymer lengths unless --no-dwell; the FASTA header and the SAM line are fprintf_fasta's and
 * fprintf_sam's (scrappie_events.c:333-344) character for character.  Here ALL files go through ONE
 * scrappie_hip_basecall_events_batch call, and the records are written in input order.  A file that cannot be read, of which nothing is
 * left after trimming, or that gives no call gets the reference's warning on stderr and no record.  Added: --model-file (weights are
 * data here; default $SCRAPPIE_MODEL_DIR/nanonet_events.scrm), --device, and --segmentation 0:p, which leaves the variance-based
 * segmentation out.  --threads is accepted (the batch is the parallel axis).  --dump (annotated events as HDF5) is not part of this
 * build and is refused.  Arguments are files; the reference's directory walk is `scrappie raw`'s here.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include "scrappie_cli.h"

static void events_usage(FILE *fh) {
    fputs("Usage: scrappie events [OPTION...] fast5 [fast5 ...]\n"
          "Scrappie basecaller -- basecall via events\n\n"
          "      --dwell, --no-dwell    Perform dwell correction of homopolymer lengths (default) / don't\n"
          "  -f, --format=format        Format to output reads (FASTA or SAM)\n"
          "  -l, --limit=nreads         Maximum number of reads to call (0 is unlimited)\n"
          "  -m, --min_prob=probability Minimum bound on probability of match\n"
          "  -o, --output=filename      Write to file rather than stdout\n"
          "  -p, --prefix=string        Prefix to append to name of each read\n"
          "  -s, --skip=penalty         Penalty for skipping a base\n"
          "  -y, --stay=penalty         Penalty for staying\n"
          "      --local=penalty        Penalty for local basecalling\n"
          "      --slip, --no-slip      Use slipping / disable slipping (default)\n"
          "      --temperature1=factor  Temperature for softmax weights\n"
          "      --temperature2=factor  Temperature for softmax bias\n"
          "  -t, --trim=start:end       Number of samples to trim, as start:end\n"
          "      --segmentation=chunk:percentile   Chunk size and percentile for variance based segmentation (chunk 0: none)\n"
          "      --uuid, --no-uuid      Output UUID / output read file (default)\n"
          "  -#, --threads=nparallel    Accepted; all files run as one batch\n"
          "      --licence, --license   Print licensing information\n"
          "      --model-file=path      Weight container (.scrm); default $SCRAPPIE_MODEL_DIR/nanonet_events.scrm\n"
          "      --device=N             GPU to run on (default 0)\n"
          "      --dump=filename        (HDF5 output of annotated events: not part of this build, refused)\n", fh);
}

int main_events(int argc, char **argv) {
    enum { O_SLIP = 256, O_NOSLIP, O_DUMP, O_DWELL, O_NODWELL, O_LOCAL, O_T1, O_T2, O_LIC, O_SEG, O_UUID, O_NOUUID, O_MFILE, O_DEV, O_H5 };
    static const struct option lo[] = {
        {"dwell", 0, 0, O_DWELL}, {"no-dwell", 0, 0, O_NODWELL}, {"format", 1, 0, 'f'}, {"limit", 1, 0, 'l'}, {"min_prob", 1, 0, 'm'},
        {"output", 1, 0, 'o'}, {"prefix", 1, 0, 'p'}, {"skip", 1, 0, 's'}, {"stay", 1, 0, 'y'}, {"local", 1, 0, O_LOCAL},
        {"temperature1", 1, 0, O_T1}, {"temperature2", 1, 0, O_T2}, {"trim", 1, 0, 't'}, {"slip", 0, 0, O_SLIP}, {"no-slip", 0, 0, O_NOSLIP},
        {"dump", 1, 0, O_DUMP}, {"licence", 0, 0, O_LIC}, {"license", 0, 0, O_LIC}, {"hdf5-compression", 1, 0, O_H5}, {"hdf5-chunk", 1, 0, O_H5},
        {"threads", 1, 0, '#'}, {"segmentation", 1, 0, O_SEG}, {"uuid", 0, 0, O_UUID}, {"no-uuid", 0, 0, O_NOUUID},
        {"model-file", 1, 0, O_MFILE}, {"device", 1, 0, O_DEV}, {"help", 0, 0, '?'}, {0, 0, 0, 0}};
    /* defaults: scrappie_events.c:108-130 */
    scrappie_hip_params p = scrappie_hip_default_params();
    p.min_prob = 1e-5f; p.skip_pen = 0.0f; p.stay_pen = 0.0f; p.local_pen = 2.0f; p.tempW = 1.0f; p.tempb = 1.0f; p.use_slip = 0;
    p.homopolymer = 0; p.want_pos = 0;
    FILE *out = stdout;
    int dwell = 1, sam = 0, limit = 0, trim_start = 200, trim_end = 10, varseg_chunk = 100, uuid_primary = 0, device = 0, c;
    float varseg_thresh = 0.0f;
    const char *prefix = "", *model_file = NULL;
    double pct;
    optind = 1;
    while ((c = getopt_long(argc, argv, "f:l:m:o:p:s:y:t:#:", lo, NULL)) != -1) {
        switch (c) {
        case 'f':
            if (0 == strcasecmp("FASTA", optarg)) sam = 0;
            else if (0 == strcasecmp("SAM", optarg)) sam = 1;
            else { fprintf(stderr, "scrappie: Unrecognised format\n"); return EXIT_FAILURE; }
            break;
        case 'l': limit = atoi(optarg); if (limit < 0) { fprintf(stderr, "scrappie: --limit wants a count >= 0\n"); return EXIT_FAILURE; } break;
        case 'm': p.min_prob = (float)atof(optarg); if (!isfinite(p.min_prob) || p.min_prob < 0.0f) { fprintf(stderr, "scrappie: --min_prob wants a probability\n"); return EXIT_FAILURE; } break;
        case 'o': if (!(out = cli_open_output(optarg))) return EXIT_FAILURE; break;
        case 'p': prefix = optarg; break;
        case 's': p.skip_pen = (float)atof(optarg); break;
        case 'y': p.stay_pen = (float)atof(optarg); break;
        case 't': if (cli_parse_trim(optarg, &trim_start, &trim_end)) { fprintf(stderr, "scrappie: --trim wants start:end, both >= 0\n"); return EXIT_FAILURE; } break;
        case '#': break;
        case O_SLIP: p.use_slip = 1; break;
        case O_NOSLIP: p.use_slip = 0; break;
        case O_DUMP: fprintf(stderr, "scrappie: --dump (annotated events as HDF5) is not part of this build\n"); return EXIT_FAILURE;
        case O_H5: break;                  /* (options of --dump) */
        case O_DWELL: dwell = 1; break;
        case O_NODWELL: dwell = 0; break;
        case O_LOCAL: p.local_pen = (float)atof(optarg); break;
        case O_T1: p.tempW = (float)atof(optarg); if (!(p.tempW > 0.0f) || !isfinite(p.tempW)) { fprintf(stderr, "scrappie: --temperature1 wants a factor > 0\n"); return EXIT_FAILURE; } break;
        case O_T2: p.tempb = (float)atof(optarg); if (!(p.tempb > 0.0f) || !isfinite(p.tempb)) { fprintf(stderr, "scrappie: --temperature2 wants a factor > 0\n"); return EXIT_FAILURE; } break;
        case O_LIC: cli_licence(); break;
        case O_SEG:
            if (cli_parse_segmentation(optarg, &varseg_chunk, &pct) || varseg_chunk < 0) { fprintf(stderr, "scrappie: --segmentation should be of form chunk:percentile\n"); return EXIT_FAILURE; }
            varseg_thresh = (float)(pct / 100.0); break;
        case O_UUID: uuid_primary = 1; break;
        case O_NOUUID: uuid_primary = 0; break;
        case O_MFILE: model_file = optarg; break;
        case O_DEV: device = atoi(optarg); break;
        default: events_usage(c == '?' && optopt == 0 ? stdout : stderr); return c == '?' && optopt == 0 ? EXIT_SUCCESS : EXIT_FAILURE;
        }
    }
    int nfile = argc - optind;
    if (nfile < 1) { events_usage(stderr); return EXIT_FAILURE; }
    if (limit > 0 && nfile > limit) nfile = limit;
    char **files = argv + optind;
    char *mpath = cli_model_path("nanonet_events", model_file);
    if (!mpath) return EXIT_FAILURE;
    raw_table *reads = calloc((size_t)nfile, sizeof *reads);
    scrappie_hip_call *calls = calloc((size_t)nfile, sizeof *calls);
    if (!reads || !calls) { fprintf(stderr, "scrappie: out of memory\n"); return EXIT_FAILURE; }
    for (int i = 0; i < nfile; i++) reads[i] = cli_load_read(files[i], trim_start, trim_end, varseg_chunk, varseg_thresh, 0);      /* (.raw NULL: no events, no call, and the warning below) */
    int model;
    scrappie_hip_engine *e = cli_open_model(device, "nanonet_events", mpath, &model);
    free(mpath);
    if (!e) return EXIT_FAILURE;
    /* the batch takes the reads that are there; the others keep their place in the output order */
    int nlive = 0;
    raw_table *live = calloc((size_t)nfile, sizeof *live);
    int *where = calloc((size_t)nfile, sizeof *where);
    if (!live || !where) { fprintf(stderr, "scrappie: out of memory\n"); return EXIT_FAILURE; }
    for (int i = 0; i < nfile; i++) if (reads[i].raw) { live[nlive] = reads[i]; where[nlive++] = i; }
    scrappie_hip_call *lc = calloc((size_t)(nlive ? nlive : 1), sizeof *lc);
    int rc = EXIT_SUCCESS;
    if (nlive && scrappie_hip_basecall_events_batch(e, model, live, (size_t)nlive, &event_detection_defaults, &p, dwell, lc)) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        for (int k = 0; k < nlive; k++) calls[where[k]] = lc[k];
        for (int i = 0; i < nfile; i++) {
            const scrappie_hip_call *res = &calls[i];
            if (!res->basecall) { fprintf(stderr, "scrappie: No basecall returned for %s\n", files[i]); continue; }
            const char *uuid = reads[i].uuid ? reads[i].uuid : "";
            char *readname = cli_record_name(files[i], NULL, 0), *id = cli_record_name(files[i], uuid, uuid_primary);
            const size_t nev = res->nblock, nbase = strlen(res->basecall);
            if (sam)
                fprintf(out, "%s%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*\n", prefix, id, res->basecall);
            else
                fprintf(out, ">%s%s  { \"filename\" : \"%s\", \"uuid\" : \"%s\", \"normalised_score\" : %f,  \"nevent\" : %zu,  \"sequence_length\" : %zu,  \"events_per_base\" : %f }\n%s\n",
                        prefix, id, readname, uuid, -res->score / nev, nev, nbase, (float)nev / (float)nbase, res->basecall);
            free(readname); free(id);
        }
        scrappie_hip_free_calls(calls, (size_t)nfile);
    }
    for (int i = 0; i < nfile; i++) { free(reads[i].raw); free(reads[i].uuid); }
    free(reads); free(calls); free(live); free(where); free(lc);
    scrappie_hip_engine_destroy(e);
    if (out != stdout) fclose(out);
    return rc;
}
