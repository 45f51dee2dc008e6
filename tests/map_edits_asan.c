/* Stand-alone driver of the host side of the transducer edit kernels (csrc/sh_host.c: scrappie_hip_map_edits_plan,
 * scrappie_hip_map_edits_pitch, scrappie_hip_map_edits_row_bytes, scrappie_hip_map_edits_max_bases) for a sanitizer build
 * (tests/test_map_edits_cpu.py).  seqlen, nblock, pitch, rows and res live in arrays of exactly n entries: a read or a write past
 * them is the sanitizer's to report.  Every plan is checked as the kernels rely on it: a row holds the n = L - k + 1 cells and slot n
 * behind them, rows and results start on 16 bytes, and what one read writes -- two matrices of nblock + 1 rows, 9 L + 4 results --
 * ends before the next read's begins and inside the buffers' sizes. */
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

static int check(const size_t *len, const size_t *nb, size_t n, size_t k) {
    int *pitch = malloc((n ? n : 1) * sizeof *pitch);
    long long *rows = malloc((n ? n : 1) * sizeof *rows), *res = malloc((n ? n : 1) * sizeof *res);
    if (!pitch || !rows || !res) return 2;
    memset(pitch, 0x7f, n * sizeof *pitch);
    memset(rows, 0x7f, n * sizeof *rows);
    memset(res, 0x7f, n * sizeof *res);
    long long nres = -1;
    const long long nrow = scrappie_hip_map_edits_plan(len, nb, n, k, pitch, rows, res, &nres);
    long long row_end = 0, res_end = 0;
    int rc = 0;
    for (size_t j = 0; j < n && !rc; j++) {
        const size_t ns = len[j] - k + 1;
        if (pitch[j] < 0 || (size_t)pitch[j] < ns + 1 || pitch[j] % 16 || (size_t)pitch[j] != scrappie_hip_map_edits_pitch(len[j], k)) rc = 3;
        if (rows[j] % 4 || res[j] % 4) rc = 4;
        if (rows[j] < row_end || res[j] < res_end) rc = 5;                        /* behind the read before */
        const long long mat = (long long)(nb[j] + 1) * pitch[j];
        if ((size_t)(2 * mat * 4) != scrappie_hip_map_edits_row_bytes(len[j], k, nb[j])) rc = 6;
        row_end = rows[j] + 2 * mat;                                              /* the last float k_map_edits_rows stores: G's last row, slot n */
        res_end = res[j] + 9 * (long long)len[j] + 4;
    }
    if (!rc && (row_end > nrow || res_end > nres)) rc = 7;
    if (!rc && n == 0 && (nrow != 0 || nres != 0)) rc = 8;
    free(pitch); free(rows); free(res);
    return rc;
}

int main(void) {
    for (size_t k = 1; k <= 5; k++) {
        const size_t maxb = scrappie_hip_map_edits_max_bases(k);
        if (maxb < k || 12 * (maxb - k + 1) + 16 > SH_MAP_LDS || 12 * (maxb - k + 2) + 16 <= SH_MAP_LDS) return 10;
        for (size_t n = 0; n <= 48; n++) {
            size_t *len = malloc((n ? n : 1) * sizeof *len), *nb = malloc((n ? n : 1) * sizeof *nb);
            if (!len || !nb) return 2;
            for (int round = 0; round < 4; round++) {
                for (size_t j = 0; j < n; j++) {
                    const size_t r = rnd(8);
                    len[j] = r == 0 ? k + rnd(3) : r == 1 ? k + 13 + rnd(4) : r == 2 ? maxb - rnd(8) : k + rnd(800);
                    nb[j] = r == 3 ? 1 : 1 + rnd(1000);
                }
                const int rc = check(len, nb, n, k);
                if (rc) { printf("k %zu, %zu reads: %d\n", k, n, rc); return rc; }
            }
            free(len); free(nb);
        }
    }
    /* nothing is read or written with a null array, res_floats may be NULL, and a read without a state is refused before any write */
    size_t len2[2] = { 9, 730 }, nb2[2] = { 3, 800 }, len3[2] = { 9, 4 };
    int pitch2[2] = { -7, -7 };
    long long rows2[2] = { -7, -7 }, res2[2] = { -7, -7 }, nres = 7;
    if (scrappie_hip_map_edits_plan(NULL, nb2, 2, 5, pitch2, rows2, res2, &nres) != 0 || nres != 0) return 21;
    if (scrappie_hip_map_edits_plan(len2, NULL, 2, 5, pitch2, rows2, res2, NULL) != 0 || scrappie_hip_map_edits_plan(len2, nb2, 2, 5, NULL, rows2, res2, NULL) != 0 ||
        scrappie_hip_map_edits_plan(len2, nb2, 2, 5, pitch2, NULL, res2, NULL) != 0 || scrappie_hip_map_edits_plan(len2, nb2, 2, 5, pitch2, rows2, NULL, NULL) != 0) return 22;
    if (scrappie_hip_map_edits_plan(len3, nb2, 2, 5, pitch2, rows2, res2, &nres) != -1 || nres != 0 || pitch2[0] != -7 || rows2[0] != -7 || res2[0] != -7) return 23;
    if (scrappie_hip_map_edits_plan(len2, nb2, 2, 0, pitch2, rows2, res2, NULL) != -1) return 24;
    if (scrappie_hip_map_edits_plan(len2, nb2, 2, 5, pitch2, rows2, res2, NULL) != 2 * 4 * 16 + 2 * 801 * 736) return 25;
    if (pitch2[0] != 16 || pitch2[1] != 736 || rows2[0] != 0 || rows2[1] != 128 || res2[0] != 0 || res2[1] != 88) return 26;
    if (scrappie_hip_map_edits_pitch(4, 5) != 0 || scrappie_hip_map_edits_row_bytes(4, 5, 10) != 0 || scrappie_hip_map_edits_max_bases(0) != 0) return 27;
    printf("ok\n");
    return 0;
}
