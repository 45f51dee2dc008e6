/* Stand-alone driver of the host side of the CRF mapping (csrc/sh_host.c: scrappie_hip_map_crf_bounds_sane,
 * scrappie_hip_map_crf_diagonal_band) for a sanitizer build (tests/test_map_crf_cpu.py).  Every band lives in arrays of exactly
 * nblock + 1 entries: a read or a write past them is the sanitizer's to report. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "scrappie_hip.h"
#include "sh_internal.h"

int main(void) {
    static const size_t NB[] = { 1, 2, 3, 7, 40, 173, 800 };
    static const size_t HW[] = { 0, 1, 2, 5, 64, (size_t)-1 };
    for (size_t a = 0; a < sizeof NB / sizeof NB[0]; a++) {
        const size_t nb = NB[a];
        size_t *low = malloc((nb + 1) * sizeof *low), *high = malloc((nb + 1) * sizeof *high);
        if (!low || !high) return 2;
        for (size_t L = 1; L <= nb + 1; L += (nb > 100 ? 37 : 1)) {
            for (size_t b = 0; b < sizeof HW / sizeof HW[0]; b++) {
                memset(low, 0xff, (nb + 1) * sizeof *low);
                memset(high, 0xff, (nb + 1) * sizeof *high);
                if (scrappie_hip_map_crf_diagonal_band(nb, L, HW[b], low, high) != 0) return 3;
                if (!scrappie_hip_map_crf_bounds_sane(low, high, nb, L)) return 4;
                for (size_t t = 0; t <= nb; t++) {
                    const size_t d = t * L / nb;
                    if (low[t] > d || d >= high[t]) return 5;
                }
                /* each way to be invalid, on a copy of exactly the same size */
                const size_t keep = high[nb];
                high[nb] = L;
                if (scrappie_hip_map_crf_bounds_sane(low, high, nb, L)) return 6;
                high[nb] = L + 2;
                if (scrappie_hip_map_crf_bounds_sane(low, high, nb, L)) return 6;
                high[nb] = keep;
                low[0] = 1;
                if (scrappie_hip_map_crf_bounds_sane(low, high, nb, L)) return 7;
                low[0] = 0;
                const size_t mid = nb / 2, kl = low[mid];
                low[mid] = high[mid];
                if (scrappie_hip_map_crf_bounds_sane(low, high, nb, L)) return 8;
                low[mid] = kl;
                if (!scrappie_hip_map_crf_bounds_sane(low, high, nb, L)) return 9;
            }
        }
        /* the full band, and what is refused before an entry is read */
        for (size_t t = 0; t <= nb; t++) { low[t] = 0; high[t] = 5; }
        if (!scrappie_hip_map_crf_bounds_sane(low, high, nb, 4)) return 10;
        if (scrappie_hip_map_crf_bounds_sane(NULL, high, nb, 4) || scrappie_hip_map_crf_bounds_sane(low, NULL, nb, 4) ||
            scrappie_hip_map_crf_bounds_sane(low, high, 0, 4) || scrappie_hip_map_crf_bounds_sane(low, high, nb, 0)) return 11;
        if (scrappie_hip_map_crf_diagonal_band(nb, 4, 1, NULL, high) != -1 || scrappie_hip_map_crf_diagonal_band(nb, 4, 1, low, NULL) != -1 ||
            scrappie_hip_map_crf_diagonal_band(0, 4, 1, low, high) != -1 || scrappie_hip_map_crf_diagonal_band(nb, 0, 1, low, high) != -1) return 12;
        free(low); free(high);
    }
    printf("ok\n");
    return 0;
}
