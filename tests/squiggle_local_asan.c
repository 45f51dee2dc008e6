/* Stand-alone driver of the window planner of the reference-local squiggle mapping (csrc/sh_host.c: scrappie_hip_squiggle_local_plan,
 * scrappie_hip_squiggle_local_stride, scrappie_hip_squiggle_local_max_cells) for a sanitizer build (tests/test_squiggle_local_cpu.py).
 * The arrays hold exactly as many entries as the call is told: a write past them is the sanitizer's to report.  Every plan is checked
 * as the kernel relies on it: every entry position 0 .. npos - 1 owned exactly once, a window's cells begin one to the left of its
 * first entry position (or at 0), reach stride - 1 + 2 (nsample - 1) past it or end at npos - 1 (inside the reference), the home
 * follows the LDS bound, scratch offsets are whole 16-byte pieces and disjoint, and the allocation covers the last window. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scrappie_hip.h"
#include "sh_internal.h"

static int check(size_t L, size_t ns, long stride, size_t cap_less) {
    long long fl0 = -1, fl = -1;
    const long long nw = scrappie_hip_squiggle_local_plan(L, ns, stride, 0, NULL, NULL, NULL, NULL, NULL, &fl0);
    if (nw <= 0) return 2;
    const size_t s = scrappie_hip_squiggle_local_stride(L, ns, stride);
    if (s == 0 || s > L) return 3;
    if ((size_t)nw != (L + s - 1) / s) return 4;
    const size_t cap = (size_t)nw > cap_less ? (size_t)nw - cap_less : 0;      /* fewer entries than windows: only they are written */
    size_t *first = malloc((cap ? cap : 1) * sizeof *first), *ncell = malloc((cap ? cap : 1) * sizeof *ncell), *own = malloc((cap ? cap : 1) * sizeof *own);
    int *home = malloc((cap ? cap : 1) * sizeof *home);
    long long *off = malloc((cap ? cap : 1) * sizeof *off);
    if (!first || !ncell || !own || !home || !off) return 5;
    int rc = 0;
    if (scrappie_hip_squiggle_local_plan(L, ns, stride, cap, first, ncell, own, home, off, &fl) != nw || fl != fl0) rc = 6;
    size_t at = 0;
    long long end = 0;
    for (size_t w = 0; w < cap && !rc; w++) {
        if (first[w] != (at ? at - 1 : 0) || own[w] == 0 || ncell[w] < own[w]) rc = 7;
        const size_t reach = at + s - 1 + 2 * (ns - 1), last = reach < L - 1 ? reach : L - 1;
        at += own[w];
        if (first[w] + ncell[w] - 1 != last || first[w] + ncell[w] > L) rc = 8;
        if (home[w] != (sh_squig_local_lds_bytes(ncell[w]) > SH_SQ_LDS)) rc = 9;
        if (!home[w]) { if (off[w] != -1) rc = 10; continue; }
        if (off[w] % 4 != 0 || off[w] < end) rc = 11;
        end = off[w] + (long long)sh_squig_local_scr_floats(ncell[w]);
        if (end > fl) rc = 13;                               /* the allocation covers every window, the last included */
    }
    if (!rc && cap == (size_t)nw && (at != L || end != fl)) rc = 12;
    free(first); free(ncell); free(own); free(home); free(off);
    return rc;
}

int main(void) {
    const size_t maxc = scrappie_hip_squiggle_local_max_cells();
    if (maxc < 4 || sh_squig_local_lds_bytes(maxc) > SH_SQ_LDS || sh_squig_local_lds_bytes(maxc + 1) <= SH_SQ_LDS) return 20;
    if (sh_squig_local_scr_lds_bytes() >= sh_squig_local_lds_bytes(1)) return 25;
    if (sh_squig_local_scr_floats(1) != 8 || sh_squig_local_scr_floats(4) != 20) return 26;
    const size_t LS[] = { 1, 2, 5, 63, 64, 65, 300, 5000, 3 * maxc + 11 };
    const size_t NSA[] = { 1, 2, 7, 64, 409, 410, 818, 819, maxc, maxc + 40 };
    const long ST[] = { 1, 7, 64, 3000, (long)maxc, (long)maxc + 1, 0, -1, -5, 1L << 40 };
    for (size_t a = 0; a < sizeof LS / sizeof LS[0]; a++)
        for (size_t b = 0; b < sizeof NSA / sizeof NSA[0]; b++)
            for (size_t c = 0; c < sizeof ST / sizeof ST[0]; c++)
                for (size_t less = 0; less < 3; less++) {
                    const int rc = check(LS[a], NSA[b], ST[c], less);
                    if (rc) { printf("npos %zu, nsample %zu, stride %ld, cap - %zu: %d\n", LS[a], NSA[b], ST[c], less, rc); return rc; }
                }
    /* nothing to cut, nothing written; the index bounds */
    size_t one = 77;
    long long fl = 5;
    if (scrappie_hip_squiggle_local_plan(0, 4, -1, 1, &one, &one, &one, NULL, NULL, &fl) != 0 || one != 77 || fl != 0) return 21;
    if (scrappie_hip_squiggle_local_plan(4, 0, -1, 1, &one, NULL, NULL, NULL, NULL, NULL) != 0 || one != 77) return 22;
    if (scrappie_hip_squiggle_local_plan(((size_t)1 << 30) + 1, 4, -1, 0, NULL, NULL, NULL, NULL, NULL, NULL) != 0) return 23;
    if (scrappie_hip_squiggle_local_plan((size_t)1 << 30, 800, -1, 0, NULL, NULL, NULL, NULL, NULL, NULL) <= 0) return 24;
    if (scrappie_hip_squiggle_local_plan((size_t)1 << 30, (size_t)1 << 30, -1, 0, NULL, NULL, NULL, NULL, NULL, NULL) <= 0) return 28;
    printf("ok\n");
    return 0;
}
