// event_fp_probe.hip -- are the divisions and square roots that event detection relies on (csrc/sh_events.h) correctly rounded
// on this GPU?  double `/`, double sqrt, float `/` and sqrtf as hipcc compiles them with the library's flags, on 2^22 random
// operands each (uniform mantissas, exponents spread over what the statistics see, denormal float quotients included),
// against the host's IEEE results bit for bit.  Prints the number of operands and of differing results per operation.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/event_fp_probe.hip -o event_fp_probe && ./event_fp_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

__global__ void k_probe(const double *a, const double *b, const float *fa, const float *fb, double *dq, double *dr, float *fq, float *fr, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dq[i] = a[i] / b[i];
    dr[i] = sqrt(a[i]);
    fq[i] = fa[i] / fb[i];
    fr[i] = sqrtf(fa[i]);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    const int n = 1 << 22;
    std::vector<double> a(n), b(n), dq(n), dr(n);
    std::vector<float> fa(n), fb(n), fq(n), fr(n);
    for (int i = 0; i < n; i++) {
        a[i] = ldexp(1.0 + (double)(rnd() >> 11) / 9007199254740992.0, (int)(rnd() % 120) - 80);
        b[i] = (i & 1) ? (double)(float)(2 + rnd() % 9) : ldexp(1.0 + (double)(rnd() >> 11) / 9007199254740992.0, (int)(rnd() % 60) - 30);
        fa[i] = ldexpf(1.0f + (float)(rnd() >> 40) / 16777216.0f, (i % 7 == 0) ? -126 : (int)(rnd() % 60) - 30);      // every seventh: FLT_MIN-scale, quotients denormal
        fb[i] = (i & 1) ? (float)(2 + rnd() % 9) : ldexpf(1.0f + (float)(rnd() >> 40) / 16777216.0f, (int)(rnd() % 20) - 10);
    }
    double *da, *db, *ddq, *ddr;
    float *dfa, *dfb, *dfq, *dfr;
    CHK(hipMalloc(&da, n * 8)); CHK(hipMalloc(&db, n * 8)); CHK(hipMalloc(&ddq, n * 8)); CHK(hipMalloc(&ddr, n * 8));
    CHK(hipMalloc(&dfa, n * 4)); CHK(hipMalloc(&dfb, n * 4)); CHK(hipMalloc(&dfq, n * 4)); CHK(hipMalloc(&dfr, n * 4));
    CHK(hipMemcpy(da, a.data(), n * 8, hipMemcpyHostToDevice)); CHK(hipMemcpy(db, b.data(), n * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(dfa, fa.data(), n * 4, hipMemcpyHostToDevice)); CHK(hipMemcpy(dfb, fb.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe, dim3((n + 255) / 256), dim3(256), 0, 0, da, db, dfa, dfb, ddq, ddr, dfq, dfr, n);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(dq.data(), ddq, n * 8, hipMemcpyDeviceToHost)); CHK(hipMemcpy(dr.data(), ddr, n * 8, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(fq.data(), dfq, n * 4, hipMemcpyDeviceToHost)); CHK(hipMemcpy(fr.data(), dfr, n * 4, hipMemcpyDeviceToHost));
    long bad[4] = {0, 0, 0, 0}, denorm = 0;
    for (int i = 0; i < n; i++) {
        volatile double hq = a[i] / b[i], hr = sqrt(a[i]);
        volatile float gq = fa[i] / fb[i], gr = sqrtf(fa[i]);
        double x = hq, y = hr; float u = gq, v = gr;
        bad[0] += memcmp(&x, &dq[i], 8) != 0; bad[1] += memcmp(&y, &dr[i], 8) != 0;
        bad[2] += memcmp(&u, &fq[i], 4) != 0; bad[3] += memcmp(&v, &fr[i], 4) != 0;
        denorm += u != 0.0f && fabsf(u) < 1.17549435e-38f;
    }
    printf("operands per operation: %d (float quotients that are denormal: %ld)\n", n, denorm);
    printf("double divide: %ld differ from the host's\ndouble sqrt:   %ld differ\nfloat divide:  %ld differ\nfloat sqrt:    %ld differ\n", bad[0], bad[1], bad[2], bad[3]);
    return (bad[0] || bad[1] || bad[2] || bad[3]) ? 3 : 0;
}
