/* scrappie_event_table.c -- the `scrappie event_table` command line over libscrappie_hip.so (src/scrappie_event_table.c).
 *
 * Same options, defaults and output as the reference's subcommand: every file is read in pA (read_raw(file, true)), trimmed and
 * segmented (trim_and_segment_raw: --trim 200:10, --segmentation 100:0), and its events are printed as
 *     # file / #event start mean stdv dwell / one line per event.
 * Here the events of ALL files come from ONE scrappie_hip_detect_events_batch call, and the tables are written in input order.  A
 * file that cannot be read, of which nothing is left after trimming, or in which no event is found gets the reference's warning on
 * stderr and no output.  Added: --device, and --segmentation 0:p, which leaves the variance-based segmentation out (the reference
 * divides by the chunk size).
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>

#include "scrappie_cli.h"

static void event_table_usage(FILE *fh) {
    fputs("Usage: scrappie event_table [OPTION...] fast5 [fast5 ...]\n"
          "Scrappie basecaller -- event detection\n\n"
          "  -o, --output=filename      Write to file rather than stdout\n"
          "  -t, --trim=start:end       Number of samples to trim, as start:end\n"
          "      --segmentation=chunk:percentile   Chunk size and percentile for variance based segmentation (chunk 0: none)\n"
          "      --licence, --license   Print licensing information\n"
          "      --device=N             GPU to run on (default 0)\n"
          "The events of all files are detected in one batched engine call and written in input order.\n", fh);
}

int main_event_table(int argc, char **argv) {
    enum { O_SEG = 256, O_LIC, O_DEV };
    static const struct option lo[] = {{"output", 1, 0, 'o'}, {"trim", 1, 0, 't'}, {"segmentation", 1, 0, O_SEG}, {"licence", 0, 0, O_LIC},
                                       {"license", 0, 0, O_LIC}, {"device", 1, 0, O_DEV}, {"help", 0, 0, '?'}, {0, 0, 0, 0}};
    /* defaults: scrappie_event_table.c:55-62 */
    FILE *out = stdout;
    int trim_start = 200, trim_end = 10, varseg_chunk = 100, device = 0, c;
    float varseg_thresh = 0.0f;
    double pct;
    optind = 1;
    while ((c = getopt_long(argc, argv, "o:t:", lo, NULL)) != -1) {
        switch (c) {
        case 'o': if (!(out = cli_open_output(optarg))) return EXIT_FAILURE; break;
        case 't': if (cli_parse_trim(optarg, &trim_start, &trim_end)) { fprintf(stderr, "scrappie: --trim wants start:end, both >= 0\n"); return EXIT_FAILURE; } break;
        case O_SEG:
            if (cli_parse_segmentation(optarg, &varseg_chunk, &pct) || varseg_chunk < 0) { fprintf(stderr, "scrappie: --segmentation should be of form chunk:percentile\n"); return EXIT_FAILURE; }
            varseg_thresh = (float)(pct / 100.0); break;
        case O_LIC: cli_licence(); break;
        case O_DEV: device = atoi(optarg); break;
        default: event_table_usage(c == '?' && optopt == 0 ? stdout : stderr); return c == '?' && optopt == 0 ? EXIT_SUCCESS : EXIT_FAILURE;
        }
    }
    const int nfile = argc - optind;
    if (nfile < 1) { event_table_usage(stderr); return EXIT_FAILURE; }
    char **files = argv + optind;
    raw_table *reads = calloc((size_t)nfile, sizeof *reads);
    scrappie_hip_event_result *res = calloc((size_t)nfile, sizeof *res);
    if (!reads || !res) { fprintf(stderr, "scrappie: out of memory\n"); return EXIT_FAILURE; }
    for (int i = 0; i < nfile; i++) reads[i] = cli_load_read(files[i], trim_start, trim_end, varseg_chunk, varseg_thresh, 0);      /* (.raw NULL: the batch refuses the read, and it is warned about below) */
    scrappie_hip_engine *e = scrappie_hip_engine_create(device);
    if (!e) { fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error()); return EXIT_FAILURE; }
    int rc = EXIT_SUCCESS;
    if (scrappie_hip_detect_events_batch(e, reads, (size_t)nfile, &event_detection_defaults, res)) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        for (int i = 0; i < nfile; i++) {
            const event_table et = res[i].events;
            if (!et.event) { fprintf(stderr, "scrappie: No events returned for %s\n", files[i]); continue; }
            fprintf(out, "# %s\n", files[i]);
            fprintf(out, "#event\tstart\tmean\tstdv\tdwell\n");
            for (size_t k = 0; k < et.n; k++)
                fprintf(out, "%zu\t%zu\t%f\t%f\t%d\n", k, (size_t)et.event[k].start, et.event[k].mean, et.event[k].stdv, (int)et.event[k].length);
        }
        scrappie_hip_free_event_results(res, (size_t)nfile);
    }
    for (int i = 0; i < nfile; i++) { free(reads[i].raw); free(reads[i].uuid); }
    free(reads); free(res);
    scrappie_hip_engine_destroy(e);
    if (out != stdout) fclose(out);
    return rc;
}
