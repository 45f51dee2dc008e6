/* Stand-alone driver of the planner that packs motifs for k_crf_find (csrc/sh_host.c: scrappie_hip_crf_find_plan,
 * scrappie_hip_crf_find_max_cells) for a sanitizer build (tests/test_crf_find_cpu.py).  The arrays hold exactly as many entries as
 * the call is told: a write past them is the sanitizer's to report.  Every plan is checked as the kernel relies on it: packs in
 * input order, a pack begins at cell 5 (behind the read's own five), a motif of L bases takes L + 4 cells, no pack passes
 * pack_cells unless it holds one motif alone, none passes the maximum, and a motif over the maximum (or empty) gets -1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scrappie_hip.h"
#include "sh_internal.h"

static int check(const size_t *len, size_t n, size_t pack_cells) {
    const size_t maxc = scrappie_hip_crf_find_max_cells();
    int *pack = malloc((n ? n : 1) * sizeof *pack);
    long long *cell = malloc((n ? n : 1) * sizeof *cell);
    if (!pack || !cell) return 2;
    const long np = scrappie_hip_crf_find_plan(len, n, pack_cells, pack, cell);
    const size_t lim = pack_cells < maxc ? pack_cells : maxc;
    int rc = 0, cur = -1, alone = 0;
    long long used = 0;
    for (size_t k = 0; k < n && !rc; k++) {
        const int over = len[k] == 0 || len[k] + 9 > maxc;
        if (over) { if (pack[k] != -1 || cell[k] != -1) rc = 3; continue; }
        if (pack[k] == cur + 1) {                         /* a new pack: the one before was full for this motif */
            if (cur >= 0 && (size_t)used + len[k] + 4 <= lim) rc = 4;
            cur = pack[k]; used = 5; alone = 1;
        } else if (pack[k] != cur) rc = 5;
        else alone = 0;
        if (cell[k] != used) rc = 6;
        used += (long long)len[k] + 4;
        if ((size_t)used > maxc) rc = 7;
        if ((size_t)used > lim && !alone) rc = 8;
        if (sh_crf_find_lds_bytes((size_t)used, 1) > SH_MAP_LDS) rc = 9;
    }
    if (!rc && np != (long)(cur + 1)) rc = 10;
    free(pack); free(cell);
    return rc;
}

int main(void) {
    const size_t maxc = scrappie_hip_crf_find_max_cells();
    if (maxc < 16 || sh_crf_find_lds_bytes(maxc, 1) > SH_MAP_LDS || sh_crf_find_lds_bytes(maxc + 1, 1) <= SH_MAP_LDS) return 20;
    if (sh_crf_find_lds_bytes(maxc, 0) > sh_crf_find_lds_bytes(maxc, 1)) return 21;
    const size_t PC[] = { 0, 1, 5, 14, 64, 128, 255, 256, 257, 1024, maxc - 1, maxc, maxc + 1, (size_t)1 << 40 };
    size_t len[400];
    unsigned long long x = 88172645463325252ull;
    for (int trial = 0; trial < 60; trial++) {
        const size_t n = trial < 2 ? (size_t)trial : 1 + (size_t)(trial * 7) % 400;
        for (size_t k = 0; k < n; k++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const unsigned r = (unsigned)(x >> 33);
            len[k] = r % 11 == 0 ? maxc - 12 + r % 8 : r % 13 == 0 ? 0 : 1 + r % (trial % 3 == 0 ? 60 : 300);
        }
        for (size_t c = 0; c < sizeof PC / sizeof PC[0]; c++) {
            const int rc = check(len, n, PC[c]);
            if (rc) { printf("trial %d (%zu motifs), pack_cells %zu: %d\n", trial, n, PC[c], rc); return rc; }
        }
    }
    /* 24 motifs of 40 bases at the default: five of 44 cells behind the read's five make 225 <= 256 */
    for (size_t k = 0; k < 24; k++) len[k] = 40;
    int pack[24];
    long long cell[24];
    if (scrappie_hip_crf_find_plan(len, 24, 256, pack, cell) != 5 || pack[4] != 0 || pack[5] != 1 || cell[4] != 5 + 4 * 44 || cell[5] != 5) return 22;
    /* null arguments: nothing is written */
    if (scrappie_hip_crf_find_plan(NULL, 3, 256, pack, cell) != 0 || scrappie_hip_crf_find_plan(len, 3, 256, NULL, cell) != 0 ||
        scrappie_hip_crf_find_plan(len, 3, 256, pack, NULL) != 0) return 23;
    printf("ok\n");
    return 0;
}
