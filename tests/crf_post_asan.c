/* Stand-alone driver of the host side of the batched CRF posterior (csrc/sh_host.c: scrappie_hip_crf_post_plan, sh_crf_post_ok,
 * sh_crf_post_stage, sh_crf_post_take) for a sanitizer build (tests/test_crf_post_cpu.py).  Matrices live in buffers that end at their last
 * column's 25th float, the staging buffer has exactly the floats the staging reports, the result buffer exactly the plan's total: a read or
 * a write past any of them is the sanitizer's to report. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scrappie_hip.h"
#include "sh_internal.h"

#define NREAD 19

int main(void) {
    /* the plan: aligned starts, no room for a read without blocks, nothing for an empty call or null arguments */
    const size_t lens[6] = { 1, 0, 7, 8, 800, 3 };
    long long off[6];
    const long long tot = scrappie_hip_crf_post_plan(lens, 6, off);
    for (int i = 0; i < 6; i++) if (off[i] % 4 || off[i] < 0) return 2;
    if (off[2] != off[1] || tot < off[5] + 4 * 5 || scrappie_hip_crf_post_plan(NULL, 0, NULL) != 0 || scrappie_hip_crf_post_plan(NULL, 3, off) != -1) return 3;

    /* 19 matrices (a full tile and three lanes) of 1 .. 37 blocks and strides 25, 28 and 32, shortest first; staged longest first */
    _Mat mats[NREAD];
    const_scrappie_matrix ptr[NREAD];
    size_t order[NREAD], nb[32];
    for (int i = 0; i < NREAD; i++) {
        const size_t nc = 1 + 2 * (size_t)i, stride = i % 3 == 0 ? 25 : (i % 3 == 1 ? 28 : 32), nfl = (nc - 1) * stride + 25;
        float *buf = malloc(nfl * sizeof(float));
        if (!buf) return 4;
        for (size_t k = 0; k < nfl; k++) buf[k] = (float)i + 0.001f * (float)k;
        mats[i].nr = 25; mats[i].nrq = 7; mats[i].nc = nc; mats[i].stride = stride; mats[i].data.f = buf;
        ptr[i] = &mats[i];
        order[i] = (size_t)(NREAD - 1 - i);
        if (!sh_crf_post_ok(ptr[i])) return 5;
    }
    _Mat bad = mats[0];
    bad.nr = 24;
    if (sh_crf_post_ok(&bad) || sh_crf_post_ok(NULL)) return 6;
    bad = mats[0]; bad.nc = 0;
    if (sh_crf_post_ok(&bad)) return 6;

    long long foff[32];
    int stride[32], T[32], tile_T[2];
    const size_t need = sh_crf_post_stage(ptr, order, NREAD, 32, NULL, foff, stride, T, tile_T);
    float *dst = malloc(need * sizeof(float));
    if (!dst || need % 2) return 7;
    if (sh_crf_post_stage(ptr, order, NREAD, 32, dst, foff, stride, T, tile_T) != need) return 8;
    if (tile_T[0] != 37 || tile_T[1] != 5 || T[0] != 37 || T[18] != 1 || T[19] != 0 || T[31] != 0) return 9;
    for (int k = 0; k < NREAD; k++) {
        const _Mat *m = ptr[order[k]];
        if (stride[k] != (int)m->stride || T[k] != (int)m->nc || foff[k] < 0 || (size_t)foff[k] + ((size_t)T[k] - 1) * m->stride + 25 > need) return 10;
        for (size_t c = 0; c < m->nc; c++) if (memcmp(dst + foff[k] + c * m->stride, m->data.f + c * m->stride, 25 * sizeof(float))) return 11;
    }

    /* results out of a buffer of exactly the plan's total */
    for (int k = 0; k < 32; k++) nb[k] = (size_t)T[k];
    long long ooff[32];
    const long long ntot = scrappie_hip_crf_post_plan(nb, 32, ooff);
    float *res = malloc((size_t)ntot * sizeof(float));
    if (!res) return 12;
    for (long long k = 0; k < ntot; k++) res[k] = (float)k;
    for (int k = 0; k < NREAD; k++) {
        scrappie_matrix p = sh_crf_post_take(res + ooff[k], nb[k]);
        if (!p || p->nr != 5 || p->nc != nb[k] + 1) return 13;
        for (size_t c = 0; c <= nb[k]; c++) for (int s = 0; s < 5; s++) if (p->data.f[c * p->stride + s] != (float)(ooff[k] + (long long)(c * 5) + s)) return 14;
        free_scrappie_matrix(p);
    }
    free(res); free(dst);
    for (int i = 0; i < NREAD; i++) free(mats[i].data.f);
    printf("ok\n");
    return 0;
}
