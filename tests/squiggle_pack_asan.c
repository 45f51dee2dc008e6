/* Stand-alone driver of the packing of candidate squiggles (csrc/sh_host.c: scrappie_hip_squiggle_pack_plan,
 * scrappie_hip_squiggle_pack_max_cells, scrappie_hip_squiggle_pack_layout) for a sanitizer build
 * (tests/test_squiggle_pack_cpu.py).  npos, pack, cell and the piece arrays live in arrays of exactly ncand entries, the cell
 * words in arrays of exactly the pack's cells: a read or a write past them is the sanitizer's to report.  Every plan is checked
 * as k_squig_pack relies on it: packs in input order, a candidate's cells directly after its predecessor's in the same pack,
 * no pack beyond pack_cells unless it holds one candidate, none beyond the most a pack may hold, -1 exactly for the candidates
 * too long for any; and every pack's END pieces: a candidate's pieces are consecutive, cover exactly its cells, each piece lies
 * inside one group of 64 cells and is headed by its first cell, at most ceil(npos / 64) + 1 per candidate, and the LDS the pack
 * takes fits. */
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

static int check_pack(const size_t *len, size_t n, const int *pack, const long long *cell, int which) {
    size_t ncell = 0, ncand = 0;
    for (size_t k = 0; k < n; k++) if (pack[k] == which) { ncell += len[k]; ncand++; }
    int *wa = malloc((ncell ? ncell : 1) * sizeof *wa), *wb = malloc((ncell ? ncell : 1) * sizeof *wb);
    int *p0 = malloc((n ? n : 1) * sizeof *p0), *np = malloc((n ? n : 1) * sizeof *np);
    if (!wa || !wb || !p0 || !np) return 2;
    for (size_t k = 0; k < n; k++) p0[k] = np[k] = -5;
    const size_t npiece = scrappie_hip_squiggle_pack_layout(len, n, pack, which, wa, wb, p0, np);
    int rc = 0;
    size_t j = 0, next_piece = 0;
    if (sh_squig_pack_lds_bytes(ncell, ncand, npiece) > SH_SQ_LDS) rc = 30;
    for (size_t k = 0; k < n && !rc; k++) {
        if (pack[k] != which) { if (p0[k] != -5 || np[k] != -5) rc = 31; continue; }
        const size_t f = (size_t)cell[k], L = len[k];
        if ((size_t)p0[k] != next_piece || np[k] < 1 || (size_t)np[k] > (L + 63) / 64 + 1) { rc = 32; break; }
        if ((size_t)np[k] != (f + L - 1) / 64 - f / 64 + 1) { rc = 33; break; }
        for (size_t pos = 0; pos < L && !rc; pos++) {
            const size_t g = f + pos;
            const int a = wa[g], b = wb[g];
            if ((size_t)(a & SH_SQP_POS_MASK) != pos || (size_t)((a >> SH_SQP_CAND_SHIFT) & SH_SQP_POS_MASK) != j) rc = 34;
            if (!(a & SH_SQP_POS0) != (pos != 0) || !(a & SH_SQP_POS1) != (pos != 1) || !(a & SH_SQP_RIGHT) != (pos + 2 > L)) rc = 35;
            if ((size_t)(b & SH_SQP_PIECE_MASK) != (size_t)p0[k] + (g / 64 - f / 64)) rc = 36;      /* one piece per group of 64 cells it touches */
            if (!(b & SH_SQP_HEAD) != !(pos == 0 || g % 64 == 0)) rc = 37;
        }
        next_piece += (size_t)np[k];
        j++;
    }
    if (!rc && next_piece != npiece) rc = 38;
    free(wa); free(wb); free(p0); free(np);
    return rc;
}

static int check(const size_t *len, size_t n, size_t pack_cells) {
    const size_t maxc = scrappie_hip_squiggle_pack_max_cells();
    const size_t lim = pack_cells < maxc ? pack_cells : maxc;
    int *pack = malloc((n ? n : 1) * sizeof *pack);
    long long *cell = malloc((n ? n : 1) * sizeof *cell);
    if (!pack || !cell) return 2;
    memset(pack, 0x7f, n * sizeof *pack);
    memset(cell, 0x7f, n * sizeof *cell);
    const long np = scrappie_hip_squiggle_pack_plan(len, n, pack_cells, pack, cell);
    long cur = -1;
    size_t used = 0;
    int rc = 0;
    for (size_t k = 0; k < n && !rc; k++) {
        const size_t c = len[k];
        if (c == 0 || c > maxc) { if (pack[k] != -1 || cell[k] != -1) rc = 3; continue; }
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
    for (long q = 0; q < np && !rc; q++) rc = check_pack(len, n, pack, cell, (int)q);
    free(pack); free(cell);
    return rc;
}

int main(void) {
    const size_t maxc = scrappie_hip_squiggle_pack_max_cells();
    if (maxc < 64 || maxc > SH_SQP_POS_MASK || sh_squig_pack_lds_bytes(maxc, maxc, maxc) > SH_SQ_LDS ||
        sh_squig_pack_lds_bytes(maxc + 1, maxc + 1, maxc + 1) <= SH_SQ_LDS) return 20;
    static const size_t PC[] = { 1, 3, 64, 128, 256, 257, 512, 1024, 4096, (size_t)-1 };
    /* a candidate that starts mid-wave, one that spans a 64-lane edge, one that spans the chunk edge at 256, and 1, 2, 3 between */
    size_t shapes[] = { 2, 1, 3, 257, 1, 63, 2, 64, 3, 65, 4, 255, 256, 40, 40, 40, 40, 40, 40, 40 };
    for (size_t a = 0; a < sizeof PC / sizeof PC[0]; a++) {
        const int rc = check(shapes, sizeof shapes / sizeof shapes[0], PC[a]);
        if (rc) { printf("pack_cells %zu, the fixed shapes: %d\n", PC[a], rc); return rc; }
    }
    for (size_t a = 0; a < sizeof PC / sizeof PC[0]; a++) {
        for (size_t n = 0; n <= 40; n++) {
            size_t *len = malloc((n ? n : 1) * sizeof *len);
            if (!len) return 2;
            for (int round = 0; round < 6; round++) {
                for (size_t k = 0; k < n; k++) {
                    const size_t r = rnd(10);
                    len[k] = r == 0 ? maxc - 1 + rnd(3) : r == 1 ? rnd(4) : r < 6 ? 1 + rnd(70) : 1 + rnd(700);
                }
                const int rc = check(len, n, PC[a]);
                if (rc) { printf("pack_cells %zu, %zu candidates: %d\n", PC[a], n, rc); return rc; }
            }
            free(len);
        }
    }
    /* the edge of a pack: maxc positions are packed, one more is not; nothing is read with no candidates or a null array */
    size_t len2[2] = { maxc, maxc + 1 };
    int pack2[2];
    long long cell2[2];
    if (scrappie_hip_squiggle_pack_plan(len2, 2, maxc, pack2, cell2) != 1 || pack2[0] != 0 || cell2[0] != 0 || pack2[1] != -1) return 21;
    if (scrappie_hip_squiggle_pack_plan(len2, 0, 256, pack2, cell2) != 0) return 22;
    if (scrappie_hip_squiggle_pack_plan(NULL, 2, 256, pack2, cell2) != 0 || scrappie_hip_squiggle_pack_plan(len2, 2, 256, NULL, cell2) != 0 ||
        scrappie_hip_squiggle_pack_plan(len2, 2, 256, pack2, NULL) != 0) return 23;
    len2[0] = (size_t)-1; len2[1] = (size_t)-2;
    if (scrappie_hip_squiggle_pack_plan(len2, 2, 256, pack2, cell2) != 0 || pack2[0] != -1 || pack2[1] != -1) return 24;
    if (scrappie_hip_squiggle_pack_layout(NULL, 2, pack2, 0, NULL, NULL, NULL, NULL) != 0) return 25;
    printf("ok\n");
    return 0;
}
