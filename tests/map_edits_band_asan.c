/* Stand-alone driver of the host side of the banded transducer edit kernels (csrc/sh_host.c: scrappie_hip_map_path_band,
 * scrappie_hip_map_edits_band_pitch, scrappie_hip_map_edits_band_row_bytes, scrappie_hip_map_edits_band_plan) for a sanitizer build
 * (tests/test_map_edits_band_cpu.py).  A path and its band live in arrays of exactly nblock entries, the plan's arrays in exactly n: a
 * read or a write past them is the sanitizer's to report.  Every band made around a path is checked with are_bounds_sane and for the
 * path inside it; every plan as the kernels rely on it: a row holds the widest entry's cells and its slot, rows and results start on
 * 16 bytes, and what one read writes -- two matrices of nblock + 1 rows, 9 L + 4 results -- ends before the next read's begins and
 * inside the buffers' sizes; a read without a band takes the unbanded pitch. */
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

/* a path of nb blocks over ns states: lead -1s, 0 .. ns - 1 in steps of 0, 1 or 2 (the last steps as large as they must be), trail -1s; 0 where it cannot be made */
static int make_path(int *path, size_t nb, size_t ns, size_t lead, size_t trail) {
    if (lead + trail >= nb) return 0;
    const size_t body = nb - lead - trail;
    if (2 * (body - 1) < ns - 1) return 0;
    for (size_t t = 0; t < lead; t++) path[t] = -1;
    size_t pos = 0;
    for (size_t t = 0; t < body; t++) {
        path[lead + t] = (int)pos;
        const size_t left = body - 1 - t;                    /* steps still to come after the next */
        size_t step = rnd(3);
        if (left > 0 && pos + step + 2 * (left - 1) < ns - 1) step = 2;
        if (pos + step > ns - 1) step = ns - 1 - pos;
        pos += step;
    }
    if ((size_t)path[lead + body - 1] != ns - 1) return 0;
    for (size_t t = nb - trail; t < nb; t++) path[t] = -1;
    return 1;
}

static int check_plan(const size_t *len, const size_t *nb, size_t *const *lo, size_t *const *hi, size_t n, size_t k) {
    int *pitch = malloc((n ? n : 1) * sizeof *pitch);
    long long *rows = malloc((n ? n : 1) * sizeof *rows), *res = malloc((n ? n : 1) * sizeof *res);
    if (!pitch || !rows || !res) return 2;
    memset(pitch, 0x7f, n * sizeof *pitch);
    memset(rows, 0x7f, n * sizeof *rows);
    memset(res, 0x7f, n * sizeof *res);
    long long nres = -1;
    const long long nrow = scrappie_hip_map_edits_band_plan(len, nb, (const size_t *const *)lo, (const size_t *const *)hi, n, k, pitch, rows, res, &nres);
    long long row_end = 0, res_end = 0;
    int rc = 0;
    for (size_t j = 0; j < n && !rc; j++) {
        if (lo[j]) {
            size_t w = 1;
            for (size_t t = 0; t < nb[j]; t++) if (hi[j][t] - lo[j][t] > w) w = hi[j][t] - lo[j][t];
            if (pitch[j] < 0 || (size_t)pitch[j] < w + 1 || (size_t)pitch[j] > w + 16 || pitch[j] % 16) rc = 3;
            if ((size_t)pitch[j] != scrappie_hip_map_edits_band_pitch(lo[j], hi[j], nb[j])) rc = 3;
            if ((size_t)(2 * (nb[j] + 1) * pitch[j] * 4) != scrappie_hip_map_edits_band_row_bytes(lo[j], hi[j], nb[j])) rc = 6;
        } else if ((size_t)pitch[j] != scrappie_hip_map_edits_pitch(len[j], k)) rc = 9;
        if (rows[j] % 4 || res[j] % 4) rc = 4;
        if (rows[j] < row_end || res[j] < res_end) rc = 5;
        row_end = rows[j] + 2 * (long long)(nb[j] + 1) * pitch[j];
        res_end = res[j] + 9 * (long long)len[j] + 4;
    }
    if (!rc && (row_end > nrow || res_end > nres)) rc = 7;
    if (!rc && n == 0 && (nrow != 0 || nres != 0)) rc = 8;
    free(pitch); free(rows); free(res);
    return rc;
}

int main(void) {
    /* bands around paths */
    size_t made = 0;
    for (int round = 0; round < 400; round++) {
        const size_t ns = 1 + rnd(round % 4 == 0 ? 3 : 300), nb = 1 + rnd(400), lead = rnd(4), trail = rnd(4);
        int *path = malloc(nb * sizeof *path);
        size_t *lo = malloc(nb * sizeof *lo), *hi = malloc(nb * sizeof *hi);
        if (!path || !lo || !hi) return 2;
        if (make_path(path, nb, ns, lead, trail)) {
            for (size_t h = 1; h <= 8; h++) {
                if (scrappie_hip_map_path_band(path, nb, ns, h, lo, hi) != 0) { printf("path band refused: %zu states, %zu blocks\n", ns, nb); return 30; }
                if (!are_bounds_sane(lo, hi, nb, ns)) { printf("band not sane: %zu states, %zu blocks, half-width %zu\n", ns, nb, h); return 31; }
                for (size_t t = 0; t < nb; t++)
                    if (path[t] >= 0 && ((size_t)path[t] < lo[t] || (size_t)path[t] >= hi[t])) return 32;
            }
            made++;
            if (scrappie_hip_map_path_band(path, nb, ns, 0, lo, hi) != -1) return 33;
            if (ns > 1) {                                   /* what is no path */
                const int keep = path[lead];
                path[lead] = 1;
                if (scrappie_hip_map_path_band(path, nb, ns, 2, lo, hi) != -1) return 34;
                path[lead] = keep;
                path[nb - trail - 1] = (int)ns;
                if (scrappie_hip_map_path_band(path, nb, ns, 2, lo, hi) != -1) return 35;
            }
        }
        free(path); free(lo); free(hi);
    }
    if (made < 100) { printf("only %zu paths\n", made); return 36; }
    /* plans over reads with bands of their paths and reads without */
    for (size_t k = 1; k <= 5; k += 2)
        for (size_t n = 0; n <= 24; n++) {
            size_t *len = malloc((n ? n : 1) * sizeof *len), *nb = malloc((n ? n : 1) * sizeof *nb);
            size_t **lo = calloc(n ? n : 1, sizeof *lo), **hi = calloc(n ? n : 1, sizeof *hi);
            if (!len || !nb || !lo || !hi) return 2;
            for (size_t j = 0; j < n; j++) {
                const size_t ns = 1 + rnd(400);
                len[j] = ns + k - 1;
                nb[j] = ns / 2 + 1 + rnd(500);
                if (rnd(4) == 0) continue;                  /* no band */
                int *path = malloc(nb[j] * sizeof *path);
                lo[j] = malloc(nb[j] * sizeof **lo); hi[j] = malloc(nb[j] * sizeof **hi);
                if (!path || !lo[j] || !hi[j]) return 2;
                if (!make_path(path, nb[j], ns, 0, 0) || scrappie_hip_map_path_band(path, nb[j], ns, 1 + rnd(40), lo[j], hi[j]) != 0) return 37;
                free(path);
            }
            const int rc = check_plan(len, nb, lo, hi, n, k);
            if (rc) { printf("k %zu, %zu reads: %d\n", k, n, rc); return rc; }
            for (size_t j = 0; j < n; j++) { free(lo[j]); free(hi[j]); }
            free(len); free(nb); free(lo); free(hi);
        }
    /* nothing is read or written with a null array, and a read without a state is refused before any write */
    size_t len2[2] = { 9, 730 }, nb2[2] = { 3, 800 }, len3[2] = { 9, 4 };
    const size_t *none[2] = { NULL, NULL };
    int pitch2[2] = { -7, -7 };
    long long rows2[2] = { -7, -7 }, res2[2] = { -7, -7 }, nres = 7;
    if (scrappie_hip_map_edits_band_plan(NULL, nb2, none, none, 2, 5, pitch2, rows2, res2, &nres) != 0 || nres != 0) return 21;
    if (scrappie_hip_map_edits_band_plan(len2, nb2, NULL, none, 2, 5, pitch2, rows2, res2, NULL) != 0 ||
        scrappie_hip_map_edits_band_plan(len2, nb2, none, NULL, 2, 5, pitch2, rows2, res2, NULL) != 0 || pitch2[0] != -7) return 22;
    if (scrappie_hip_map_edits_band_plan(len3, nb2, none, none, 2, 5, pitch2, rows2, res2, &nres) != -1 || nres != 0 || pitch2[0] != -7 || rows2[0] != -7) return 23;
    if (scrappie_hip_map_edits_band_plan(len2, nb2, none, none, 2, 0, pitch2, rows2, res2, NULL) != -1) return 24;
    if (scrappie_hip_map_edits_band_plan(len2, nb2, none, none, 2, 5, pitch2, rows2, res2, NULL) != scrappie_hip_map_edits_plan(len2, nb2, 2, 5, pitch2, rows2, res2, NULL)) return 25;
    if (scrappie_hip_map_edits_band_pitch(NULL, NULL, 3) != 0 || scrappie_hip_map_edits_band_row_bytes(NULL, NULL, 3) != 0) return 26;
    printf("ok\n");
    return 0;
}
