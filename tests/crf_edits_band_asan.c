/* Stand-alone driver of the host side of the banded edit kernels (csrc/sh_host.c: scrappie_hip_map_crf_path_band,
 * scrappie_hip_crf_edits_band_pitch, scrappie_hip_crf_edits_band_row_bytes, scrappie_hip_crf_edits_band_plan) for a sanitizer build
 * (tests/test_crf_edits_band_cpu.py).  Paths and bands live in arrays of exactly nblock + 1 entries, the plan's arrays in exactly n: a
 * read or a write past them is the sanitizer's to report.  Every band made from a path is checked by scrappie_hip_map_crf_bounds_sane and
 * for holding the path; every plan as the kernels rely on it: a row holds the widest entry's cells and one slot more, rows and results
 * start on 16 bytes, and what one read writes ends before the next read's begins and inside the buffers' sizes. */
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

/* a random path of L bases over nb + 1 entries (L <= nb + 1): which entries are bases */
static void make_path(int *path, size_t nb, size_t L) {
    size_t left = L, cnt = 0;
    for (size_t t = 0; t <= nb; t++) {
        const size_t entries = nb + 1 - t;
        if (left && (left == entries || rnd(entries) < left)) { cnt++; left--; }
        path[t] = (int)cnt - 1;
    }
}

static int band_of(size_t nb, size_t L, size_t h, size_t **lo_out, size_t **hi_out) {
    int *path = malloc((nb + 1) * sizeof *path);
    size_t *lo = malloc((nb + 1) * sizeof *lo), *hi = malloc((nb + 1) * sizeof *hi);
    if (!path || !lo || !hi) return 2;
    make_path(path, nb, L);
    int rc = 0;
    if (scrappie_hip_map_crf_path_band(path, nb, L, h, lo, hi) != 0) rc = 31;
    if (!rc && !scrappie_hip_map_crf_bounds_sane(lo, hi, nb, L)) rc = 32;
    size_t w = 1;
    for (size_t t = 0; t <= nb && !rc; t++) {
        const size_t c = (size_t)(path[t] + 1);
        if (c < lo[t] || c >= hi[t]) rc = 33;                                     /* the path is inside */
        if (hi[t] - lo[t] > 2 * h + 1 + (t == 0)) rc = 34;                        /* (entry 0 begins at cell 0 whatever the half-width) */
        if (hi[t] - lo[t] > w) w = hi[t] - lo[t];
    }
    if (!rc) {
        const size_t p = scrappie_hip_crf_edits_band_pitch(lo, hi, nb);
        if (p < w + 1 || p % 16 || p > w + 16) rc = 35;
        if (scrappie_hip_crf_edits_band_row_bytes(lo, hi, nb) != 3 * (nb + 1) * p * 4) rc = 36;
    }
    /* what is no path is refused and nothing is written: a step of two, a step down, the wrong end, a value outside */
    if (!rc && nb >= 2) {
        const int keep = path[1];
        path[1] = path[0] + 2;
        if (scrappie_hip_map_crf_path_band(path, nb, L, h, lo, hi) != -1) rc = 37;
        path[1] = path[0] - 1;
        if (path[0] >= 0 && scrappie_hip_map_crf_path_band(path, nb, L, h, lo, hi) != -1) rc = 38;
        path[1] = keep;
        path[nb] -= 1;
        if (scrappie_hip_map_crf_path_band(path, nb, L, h, lo, hi) != -1) rc = 39;
        path[nb] += 2;
        if (scrappie_hip_map_crf_path_band(path, nb, L, h, lo, hi) != -1) rc = 40;
        path[nb] -= 1;
    }
    if (!rc && (scrappie_hip_map_crf_path_band(NULL, nb, L, h, lo, hi) != -1 || scrappie_hip_map_crf_path_band(path, nb, L, h, NULL, hi) != -1 ||
                scrappie_hip_map_crf_path_band(path, nb, L, h, lo, NULL) != -1 || scrappie_hip_map_crf_path_band(path, 0, L, h, lo, hi) != -1 ||
                scrappie_hip_map_crf_path_band(path, nb, 0, h, lo, hi) != -1)) rc = 41;
    free(path);
    if (rc) { free(lo); free(hi); return rc; }
    *lo_out = lo; *hi_out = hi;
    return 0;
}

static int check_plan(size_t n) {
    const size_t m = n ? n : 1;
    size_t *len = malloc(m * sizeof *len), *nb = malloc(m * sizeof *nb);
    size_t **lo = malloc(m * sizeof *lo), **hi = malloc(m * sizeof *hi);
    int *pitch = malloc(m * sizeof *pitch);
    long long *rows = malloc(m * sizeof *rows), *res = malloc(m * sizeof *res);
    if (!len || !nb || !lo || !hi || !pitch || !rows || !res) return 2;
    int rc = 0;
    size_t made = 0;
    for (size_t k = 0; k < n && !rc; k++, made++) {
        nb[k] = 1 + rnd(rnd(4) ? 60 : 900);
        len[k] = 1 + rnd(nb[k] + 1);
        const size_t h = rnd(5) == 0 ? 0 : rnd(5) == 1 ? len[k] + 3 : rnd(40);
        lo[k] = hi[k] = NULL;
        if (rnd(7) == 0) continue;                                                /* a read without a band */
        rc = band_of(nb[k], len[k], h, &lo[k], &hi[k]);
    }
    long long nres = -1;
    const long long nrow = rc ? 0 : scrappie_hip_crf_edits_band_plan(len, nb, (const size_t *const *)lo, (const size_t *const *)hi, n, pitch, rows, res, &nres);
    long long row_end = 0, res_end = 0;
    for (size_t k = 0; k < n && !rc; k++) {
        const size_t want = lo[k] ? scrappie_hip_crf_edits_band_pitch(lo[k], hi[k], nb[k]) : scrappie_hip_crf_edits_pitch(len[k]);
        if (pitch[k] <= 0 || (size_t)pitch[k] != want || pitch[k] % 16) rc = 3;
        if (rows[k] % 4 || res[k] % 4) rc = 4;
        if (rows[k] < row_end || res[k] < res_end) rc = 5;
        const long long mat = (long long)(nb[k] + 1) * pitch[k];
        if (lo[k] && (size_t)(3 * mat * 4) != scrappie_hip_crf_edits_band_row_bytes(lo[k], hi[k], nb[k])) rc = 6;
        row_end = rows[k] + 3 * mat;
        res_end = res[k] + 9 * (long long)len[k] + 4;
    }
    if (!rc && (row_end > nrow || res_end > nres)) rc = 7;
    if (!rc && n == 0 && (nrow != 0 || nres != 0)) rc = 8;
    for (size_t k = 0; k < made; k++) { free(lo[k]); free(hi[k]); }
    free(len); free(nb); free(lo); free(hi); free(pitch); free(rows); free(res);
    return rc;
}

int main(void) {
    for (size_t n = 0; n <= 24; n++)
        for (int round = 0; round < 6; round++) {
            const int rc = check_plan(n);
            if (rc) { printf("%zu reads: %d\n", n, rc); return rc; }
        }
    /* the corners by hand: one block; every entry a base; half-width 0 on a path whose entry 0 is a base (low[0] stays 0) */
    {
        int p1[2] = { 0, 1 };
        size_t lo[2], hi[2];
        if (scrappie_hip_map_crf_path_band(p1, 1, 2, 0, lo, hi) != 0 || lo[0] != 0 || hi[0] != 2 || lo[1] != 2 || hi[1] != 3) return 21;
        if (!scrappie_hip_map_crf_bounds_sane(lo, hi, 1, 2)) return 22;
        int p2[2] = { -1, 0 };
        if (scrappie_hip_map_crf_path_band(p2, 1, 1, 0, lo, hi) != 0 || lo[0] != 0 || hi[0] != 1 || lo[1] != 1 || hi[1] != 2) return 23;
        int p3[2] = { 1, 1 };                                                     /* two bases through entry 0: no path */
        if (scrappie_hip_map_crf_path_band(p3, 1, 2, 4, lo, hi) != -1) return 24;
        if (scrappie_hip_crf_edits_band_pitch(NULL, hi, 1) != 0 || scrappie_hip_crf_edits_band_pitch(lo, NULL, 1) != 0) return 25;
    }
    /* nothing is read or written with a null array, and res_floats may be NULL */
    {
        size_t len2[2] = { 5, 9 }, nb2[2] = { 3, 3 };
        size_t l0[4] = { 0, 0, 1, 2 }, h0[4] = { 2, 3, 5, 6 };
        const size_t *lo2[2] = { l0, NULL }, *hi2[2] = { h0, NULL };
        int pitch2[2];
        long long rows2[2], res2[2], nres = 7;
        if (scrappie_hip_crf_edits_band_plan(NULL, nb2, lo2, hi2, 2, pitch2, rows2, res2, &nres) != 0 || nres != 0) return 26;
        if (scrappie_hip_crf_edits_band_plan(len2, nb2, NULL, hi2, 2, pitch2, rows2, res2, NULL) != 0 ||
            scrappie_hip_crf_edits_band_plan(len2, nb2, lo2, NULL, 2, pitch2, rows2, res2, NULL) != 0) return 27;
        if (scrappie_hip_crf_edits_band_plan(len2, nb2, lo2, hi2, 2, pitch2, rows2, res2, NULL) != 3 * 4 * 16 + 3 * 4 * 16) return 28;
        if (pitch2[0] != 16 || pitch2[1] != 16 || rows2[0] != 0 || rows2[1] != 192 || res2[0] != 0 || res2[1] != 52) return 29;
    }
    printf("ok\n");
    return 0;
}
