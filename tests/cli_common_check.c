/* cli_common_check.c -- drives the layer the subcommands of `scrappie` share (scrappie_amd/csrc/scrappie_cli.c) from a program of its
 * own, so that it runs under the address and undefined-behaviour sanitizers with their leak check: tests/test_cli_common_cpu.py builds
 * it with scrappie_cli.c and the host C it calls, and compares what it prints.  Everything it is given it frees.
 *   trim ARG...                               one line per ARG: rc start end (start and end stay -7 where nothing is written)
 *   seg ARG...                                one line per ARG: rc chunk pct
 *   load DIR START END CHUNK PCT NORM FILE...  cli_load_read of every FILE: a line "start end n has_uuid", the window to DIR/<index>.f32
 *   model NAME [FILE]                         cli_model_path: the path, or NULL
 *   fasta LIMIT FILE...                       cli_read_fasta over the FILEs: "rc=.." per file, then name<TAB>sequence per record */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scrappie_cli.h"

/* the engine is not exercised here */
scrappie_hip_engine *scrappie_hip_engine_create(int device) { (void)device; return NULL; } void scrappie_hip_engine_destroy(scrappie_hip_engine *e) { (void)e; }
int scrappie_hip_load_model(scrappie_hip_engine *e, const char *name, const char *path) { (void)e; (void)name; (void)path; return -1; } const char *scrappie_hip_last_error(void) { return "no engine in this program"; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (0 == strcmp(argv[1], "trim")) {
        for (int i = 2; i < argc; i++) {
            int start = -7, end = -7;
            const int rc = cli_parse_trim(argv[i], &start, &end);
            printf("%d %d %d\n", rc, start, end);
        }
    } else if (0 == strcmp(argv[1], "seg")) {
        for (int i = 2; i < argc; i++) {
            int chunk = -7;
            double pct = -7.0;
            const int rc = cli_parse_segmentation(argv[i], &chunk, &pct);
            printf("%d %d %.17g\n", rc, chunk, pct);
        }
    } else if (0 == strcmp(argv[1], "load") && argc >= 8) {
        for (int i = 8; i < argc; i++) {
            raw_table rt = cli_load_read(argv[i], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), (float)(atof(argv[6]) / 100.0), atoi(argv[7]));
            printf("%zu %zu %zu %d\n", rt.start, rt.end, rt.n, rt.uuid != NULL);
            if (rt.raw) {
                char path[4096];
                snprintf(path, sizeof path, "%s/%d.f32", argv[2], i - 8);
                FILE *fh = fopen(path, "wb");
                if (!fh || fwrite(rt.raw + rt.start, sizeof(float), rt.end - rt.start, fh) != rt.end - rt.start) return 3;
                fclose(fh);
            }
            free(rt.raw); free(rt.uuid);
        }
    } else if (0 == strcmp(argv[1], "model") && argc >= 3) {
        char *path = cli_model_path(argv[2], argc > 3 ? argv[3] : NULL);
        puts(path ? path : "NULL");
        free(path);
    } else if (0 == strcmp(argv[1], "fasta") && argc >= 3) {
        struct cli_fasta *recs = NULL;
        size_t nrec = 0;
        for (int i = 3; i < argc; i++) printf("rc=%d\n", cli_read_fasta(argv[i], &recs, &nrec, (size_t)atoi(argv[2])));
        for (size_t i = 0; i < nrec; i++) printf("%s\t%s\n", recs[i].name, recs[i].seq);
        cli_free_fasta(recs, nrec);
    } else return 2;
    return 0;
}
