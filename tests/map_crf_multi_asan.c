/* Stand-alone driver of the packing of a flip-flop read's candidates (csrc/sh_host.c: scrappie_hip_map_crf_pack_plan,
 * scrappie_hip_map_crf_pack_max_cells) for a sanitizer build (tests/test_map_crf_multi_cpu.py).  seqlen, pack and cell live in arrays
 * of exactly ncand entries: a read or a write past them is the sanitizer's to report.  Every plan is checked as the kernel relies on
 * it: a candidate of L bases takes L + 1 cells, packs in input order, a candidate's cells directly after its predecessor's in the same
 * pack, no pack beyond pack_cells unless it holds one candidate, none beyond the most a pack may hold, -1 exactly for the candidates
 * too long for any. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scrappie_hip.h"
#include "sh_internal.h"

static unsigned long long rng_state = 0x2545f4914f6cdd1dull;
static size_t rnd(size_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (size_t)(rng_state % n);
}

static int check(const size_t *len, size_t n, size_t pack_cells) {
    const size_t maxc = scrappie_hip_map_crf_pack_max_cells();
    const size_t lim = pack_cells < maxc ? pack_cells : maxc;
    int *pack = malloc((n ? n : 1) * sizeof *pack);
    long long *cell = malloc((n ? n : 1) * sizeof *cell);
    if (!pack || !cell) return 2;
    memset(pack, 0x7f, n * sizeof *pack);
    memset(cell, 0x7f, n * sizeof *cell);
    const long np = scrappie_hip_map_crf_pack_plan(len, n, pack_cells, pack, cell);
    long cur = -1;
    size_t used = 0;
    int rc = 0;
    for (size_t k = 0; k < n && !rc; k++) {
        const size_t c = len[k] + 1;
        if (len[k] > maxc - 1) { if (pack[k] != -1 || cell[k] != -1) rc = 3; continue; }
        if (pack[k] < 0 || pack[k] >= np) { rc = 4; break; }
        if (pack[k] == cur) {
            if (cell[k] != (long long)used) rc = 5;               /* contiguous, disjoint */
            if (used + c > lim) rc = 6;                           /* a pack of several stays within pack_cells */
            used += c;
        } else {
            if (pack[k] != cur + 1 || cell[k] != 0) rc = 7;       /* packs in input order, each from cell 0 */
            if (cur >= 0 && used + c <= lim) rc = 8;              /* closed only when the candidate would not have fitted */
            cur = pack[k]; used = c;
        }
        if (used > maxc) rc = 9;
    }
    if (!rc && cur + 1 != np) rc = 10;
    free(pack); free(cell);
    return rc;
}

int main(void) {
    const size_t maxc = scrappie_hip_map_crf_pack_max_cells();
    if (maxc < 2 || sh_map_crf_pack_lds_bytes(maxc) > SH_MAP_LDS || sh_map_crf_pack_lds_bytes(maxc + 1) <= SH_MAP_LDS) return 20;
    static const size_t PC[] = { 1, 2, 64, 256, 257, 1024, 4096, (size_t)-1 };
    for (size_t a = 0; a < sizeof PC / sizeof PC[0]; a++) {
        for (size_t n = 0; n <= 40; n++) {
            size_t *len = malloc((n ? n : 1) * sizeof *len);
            if (!len) return 2;
            for (int round = 0; round < 6; round++) {
                for (size_t k = 0; k < n; k++) {
                    const size_t r = rnd(10);
                    len[k] = r == 0 ? maxc - 2 + rnd(3) : r == 1 ? 1 + rnd(3) : r < 6 ? 1 + rnd(60) : 1 + rnd(700);
                }
                const int rc = check(len, n, PC[a]);
                if (rc) { printf("pack_cells %zu, %zu candidates: %d\n", PC[a], n, rc); return rc; }
            }
            free(len);
        }
    }
    /* the edge of a pack: maxc - 1 bases are packed, one more is not; nothing is read with no candidates or a null array */
    size_t len2[2] = { maxc - 1, maxc };
    int pack2[2];
    long long cell2[2];
    if (scrappie_hip_map_crf_pack_plan(len2, 2, maxc, pack2, cell2) != 1 || pack2[0] != 0 || cell2[0] != 0 || pack2[1] != -1) return 21;
    if (scrappie_hip_map_crf_pack_plan(len2, 0, 256, pack2, cell2) != 0) return 22;
    if (scrappie_hip_map_crf_pack_plan(NULL, 2, 256, pack2, cell2) != 0 || scrappie_hip_map_crf_pack_plan(len2, 2, 256, NULL, cell2) != 0 ||
        scrappie_hip_map_crf_pack_plan(len2, 2, 256, pack2, NULL) != 0) return 23;
    len2[0] = (size_t)-1; len2[1] = (size_t)-2;                                   /* no overflow in seqlen + 1 */
    if (scrappie_hip_map_crf_pack_plan(len2, 2, 256, pack2, cell2) != 0 || pack2[0] != -1 || pack2[1] != -1) return 24;
    printf("ok\n");
    return 0;
}
