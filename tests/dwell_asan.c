/* Stand-alone driver of the host statements of the dwell correction (csrc/sh_host.c: homopolymer_dwell_correction,
 * dwell_corrected_overlapper) for a sanitizer build (tests/test_dwell_cpu.py).  The file given holds int32 words: the number of cases,
 * then per case nstate, n, n path entries, n dwells.  Each case runs as `scrappie events` runs a read -- overlapper with pos, the events
 * annotated, the correction -- on buffers of exactly n entries, and once through dwell_corrected_overlapper at a scale of 9; two lines
 * per case, the strings ("NULL": none).  Then the edges: paths of stays, a scale of zero, a dwell far past any reservation. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scrappie_hip.h"

static void show(char *s) {
    printf("%s\n", s ? s : "NULL");
    free(s);
}

static void run(int nstate, int n, const int *path_in, const int *dwell_in) {
    int *path = malloc((size_t)n * sizeof(int)), *dwell = malloc((size_t)n * sizeof(int)), *pos = calloc((size_t)n, sizeof(int));
    event_t *ev = malloc((size_t)n * sizeof(event_t));
    memcpy(path, path_in, (size_t)n * sizeof(int));
    memcpy(dwell, dwell_in, (size_t)n * sizeof(int));
    uint64_t at = 0;
    char *plain = overlapper(path, (size_t)n, nstate - 1, pos);
    for (int i = 0; i < n; i++) {
        ev[i].start = at; ev[i].length = (float)dwell[i]; ev[i].mean = 80.0f; ev[i].stdv = 1.0f;
        ev[i].pos = pos[i]; ev[i].state = 1 + path[i];
        at += (uint64_t)dwell[i];
    }
    const event_table et = { (size_t)n, 0, (size_t)n, ev };
    show(plain ? homopolymer_dwell_correction(et, path, (size_t)nstate, strlen(plain)) : NULL);
    const dwell_model dm = { 9.0f, { 0.0f, 0.0f, 0.0f, 0.0f } };
    show(dwell_corrected_overlapper(path, dwell, n, nstate - 1, dm));
    free(plain); free(ev); free(pos); free(dwell); free(path);
}

int main(int argc, char **argv) {
    if (argc > 1) {
        FILE *fh = fopen(argv[1], "rb");
        if (!fh) return 2;
        int ncase = 0;
        if (fread(&ncase, sizeof(int), 1, fh) != 1) return 3;
        for (int c = 0; c < ncase; c++) {
            int head[2];
            if (fread(head, sizeof(int), 2, fh) != 2 || head[1] < 1) return 3;
            int *w = malloc(2 * (size_t)head[1] * sizeof(int));
            if (fread(w, sizeof(int), 2 * (size_t)head[1], fh) != 2 * (size_t)head[1]) return 3;
            run(head[0], head[1], w, w + head[1]);
            free(w);
        }
        fclose(fh);
    }
    /* every entry a stay, lengths 1 .. 9: no call, no read before the first k-mer that is not there */
    for (int n = 1; n <= 9; n++) {
        int stays[9], dw[9];
        for (int i = 0; i < 9; i++) { stays[i] = -1; dw[i] = 5 + i; }
        run(1025, n, stays, dw);
    }
    /* AAAAA, AAAAA: a scale of zero (no int to round to) and a dwell of a million over a scale of 1/8 */
    const int homo[2] = { 0, 0 }, dz[2] = { 3, 7 }, dbig[2] = { 3, 1000000 };
    const dwell_model zero = { 0.0f, { 0.0f, 0.0f, 0.0f, 0.0f } }, small = { 0.125f, { 0.0f, 0.0f, 0.0f, 0.0f } };
    show(dwell_corrected_overlapper(homo, dz, 2, 1024, zero));
    char *big = dwell_corrected_overlapper(homo, dbig, 2, 1024, small);
    printf("%zu\n", big ? strlen(big) : (size_t)0);
    free(big);
    return 0;
}
