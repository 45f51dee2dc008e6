/* Stand-alone driver of the host side of the edit kernels (csrc/sh_host.c: scrappie_hip_crf_edits_plan, scrappie_hip_crf_edits_pitch,
 * scrappie_hip_crf_edits_row_bytes) for a sanitizer build (tests/test_crf_edits_cpu.py).  seqlen, nblock, pitch, rows and res live in
 * arrays of exactly n entries: a read or a write past them is the sanitizer's to report.  Every plan is checked as the kernels rely
 * on it: a row holds cells 0 .. L and the spare slot behind them, rows and results start on 16 bytes, and what one read writes --
 * three matrices of nblock + 1 rows, 9 L + 4 results -- ends before the next read's begins and inside the buffers' sizes. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scrappie_hip.h"
#include "sh_internal.h"

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static size_t rnd(size_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (size_t)(rng_state % n);
}

static int check(const size_t *len, const size_t *nb, size_t n) {
    int *pitch = malloc((n ? n : 1) * sizeof *pitch);
    long long *rows = malloc((n ? n : 1) * sizeof *rows), *res = malloc((n ? n : 1) * sizeof *res);
    if (!pitch || !rows || !res) return 2;
    memset(pitch, 0x7f, n * sizeof *pitch);
    memset(rows, 0x7f, n * sizeof *rows);
    memset(res, 0x7f, n * sizeof *res);
    long long nres = -1;
    const long long nrow = scrappie_hip_crf_edits_plan(len, nb, n, pitch, rows, res, &nres);
    long long row_end = 0, res_end = 0;
    int rc = 0;
    for (size_t k = 0; k < n && !rc; k++) {
        if (pitch[k] < 0 || (size_t)pitch[k] < len[k] + 2 || pitch[k] % 16 || (size_t)pitch[k] != scrappie_hip_crf_edits_pitch(len[k])) rc = 3;
        if (rows[k] % 4 || res[k] % 4) rc = 4;
        if (rows[k] < row_end || res[k] < res_end) rc = 5;                        /* behind the read before */
        const long long mat = (long long)(nb[k] + 1) * pitch[k];
        if ((size_t)(3 * mat * 4) != scrappie_hip_crf_edits_row_bytes(len[k], nb[k])) rc = 6;
        row_end = rows[k] + 3 * mat;                                              /* the last float k_crf_edits_rows stores: G_B's last row, the spare slot */
        res_end = res[k] + 9 * (long long)len[k] + 4;
    }
    if (!rc && (row_end > nrow || res_end > nres)) rc = 7;
    if (!rc && n == 0 && (nrow != 0 || nres != 0)) rc = 8;
    free(pitch); free(rows); free(res);
    return rc;
}

int main(void) {
    for (size_t n = 0; n <= 48; n++) {
        size_t *len = malloc((n ? n : 1) * sizeof *len), *nb = malloc((n ? n : 1) * sizeof *nb);
        if (!len || !nb) return 2;
        for (int round = 0; round < 8; round++) {
            for (size_t k = 0; k < n; k++) {
                const size_t r = rnd(8);
                len[k] = r == 0 ? 1 + rnd(3) : r == 1 ? 13 + rnd(4) : r == 2 ? 3255 + rnd(8) : 1 + rnd(800);
                nb[k] = r == 3 ? 1 : 1 + rnd(1000);
            }
            const int rc = check(len, nb, n);
            if (rc) { printf("%zu reads: %d\n", n, rc); return rc; }
        }
        free(len); free(nb);
    }
    /* nothing is read or written with a null array, and res_floats may be NULL */
    size_t len2[2] = { 5, 730 }, nb2[2] = { 3, 800 };
    int pitch2[2];
    long long rows2[2], res2[2], nres = 7;
    if (scrappie_hip_crf_edits_plan(NULL, nb2, 2, pitch2, rows2, res2, &nres) != 0 || nres != 0) return 21;
    if (scrappie_hip_crf_edits_plan(len2, NULL, 2, pitch2, rows2, res2, NULL) != 0 || scrappie_hip_crf_edits_plan(len2, nb2, 2, NULL, rows2, res2, NULL) != 0 ||
        scrappie_hip_crf_edits_plan(len2, nb2, 2, pitch2, NULL, res2, NULL) != 0 || scrappie_hip_crf_edits_plan(len2, nb2, 2, pitch2, rows2, NULL, NULL) != 0) return 22;
    if (scrappie_hip_crf_edits_plan(len2, nb2, 2, pitch2, rows2, res2, NULL) != 3 * 4 * 16 + 3 * 801 * 736) return 23;
    if (pitch2[0] != 16 || pitch2[1] != 736 || rows2[0] != 0 || rows2[1] != 192 || res2[0] != 0 || res2[1] != 52) return 24;
    printf("ok\n");
    return 0;
}
