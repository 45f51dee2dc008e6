/* Stand-alone driver of the host statement of detect_events (csrc/sh_host.c) for a sanitizer build (tests/test_events_cpu.py):
 * every file given (headerless float32 samples) and then every length 0 .. 40 of a generated read go through
 * scrappie_hip_detect_events_host, statistics included; one line per run: the number of events (0: no table). */
#include <stdio.h>
#include <stdlib.h>
#include "scrappie_hip.h"

static size_t run(const float *x, size_t n) {
    float *t1 = malloc((n ? n : 1) * sizeof(float)), *t2 = malloc((n ? n : 1) * sizeof(float));
    event_table et = scrappie_hip_detect_events_host(x, n, &event_detection_defaults, t1, t2);
    const size_t nev = et.event ? et.n : 0;
    double acc = 0.0;                      /* touch every byte that came back */
    for (size_t i = 0; i < nev; i++) acc += (double)et.event[i].start + et.event[i].length + et.event[i].mean + et.event[i].stdv;
    for (size_t i = 0; et.event && i < n; i++) acc += t1[i] + t2[i];
    if (acc != acc) fprintf(stderr, "nan\n");
    free(et.event); free(t1); free(t2);
    return nev;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        FILE *fh = fopen(argv[a], "rb");
        if (!fh) return 2;
        fseek(fh, 0, SEEK_END);
        const size_t n = (size_t)ftell(fh) / sizeof(float);
        fseek(fh, 0, SEEK_SET);
        float *x = malloc((n ? n : 1) * sizeof(float));
        if (fread(x, sizeof(float), n, fh) != n) return 3;
        fclose(fh);
        printf("%zu\n", run(x, n));
        free(x);
    }
    unsigned s = 12345u;
    for (size_t n = 0; n <= 40; n++) {
        float *x = malloc((n ? n : 1) * sizeof(float));      /* exactly n samples: a read past the end is a report */
        float level = 90.0f;
        for (size_t i = 0; i < n; i++) {
            s = s * 1664525u + 1013904223u;
            if ((s >> 28) < 3) level = 70.0f + (float)((s >> 8) & 63);
            x[i] = level + (float)((s >> 16) & 255) / 256.0f;
        }
        printf("%zu\n", run(x, n));
        free(x);
    }
    return 0;
}
