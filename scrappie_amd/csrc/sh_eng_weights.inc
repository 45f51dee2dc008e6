/* sh_eng_weights.inc -- part of scrappie_hip.hip (one translation unit, included from there in this order; not compiled alone):
 * weights as the device wants them: MFMA fragments, fp16 pieces, bias tables; the Model. */

/* ------------------------------------------------------------------ */
/* model                                                                */
/* ------------------------------------------------------------------ */
static ShConvGeom conv_geom(int WL, int st, int F) {      /* layers.c:169-207 */
    ShConvGeom g;
    g.WL = WL; g.st = st; g.F = F;
    g.padL = (g.WL - 1) / 2; g.padR = g.WL / 2;
    g.c0 = (g.padL + g.st - 1) / g.st;
    g.shiftX = g.c0 * g.st - g.padL;
    g.nstepC = (g.WL + g.st - 1) / g.st;
    g.nstepX = g.st * g.nstepC;
    return g;
}

struct HostMat { int nr = 0, nc = 0; std::vector<float> v; };   /* v[c*nr + r]: column c = output unit */

struct Model {
    std::string name;
    int arch = 0, conv_act = 0, stride = 5;
    int F = 0, WL = 0, S = 0, NS = 0;
    bool ff_no_clamp = false;       /* every output-layer logit is provably inside exp_ps's clamp (+-88.376): S1 inside the decoder skips the v_med3_f32 (sh_eng_load.inc) */
    ShConvGeom geom{};
    size_t min_samples = 0;
    /* device weights */
    DBuf conv_W, conv_b;                 /* [WL][F], [F] */
    DBuf iW[5], ib[5], sW[5], sW2[5];    /* fragments (fp32: exact-fp32 MFMA kernels) */
    DBuf iWp[5], sWp[5], sW2p[5], ffWp;  /* the same rows as fp16 pieces (split products: sh_kernels.h) */
    DBuf ibs[5], ffbs;                   /* biases in the split products' accumulator units (x 2^14) */
    DBuf iWp32[5], sWp32[5], sW2p32[5], ib32[5];   /* GRU layers of S = 96 for k_gru_proj32: pieces in 32-row m-tiles / 16-wide k steps, bias table */
    bool has32 = false;
    DBuf ffW, ffb;
    int ff_mtiles = 0;
    DBuf ff2W[2][2], ff2b[2];            /* raw_r94 / events: FF1/FF2 {Wf, Wb}, b (feedforward2_tanh) */
    DBuf lp[4];                          /* events: LSTM peepholes [update | forget | output] in accumulator layout */
    int nfeat = 0;                       /* events: input features per event (12), padded to F = 16 */
    DBuf sqw;                            /* arch 4 (squiggle predictor): the weight table of k_sqnet (sh_sqnet.h); WL is its window, nothing else above is set */
    bool layer_f32[5] = {false, false, false, false, false};   /* GRU layer has a weight outside the split products' range: exact-fp32 kernels */
};

/* MFMA A fragments of an (M x K) weight matrix given as rows m (output unit)
 * of K inputs: frag[(mt*(K/4) + r)*64 + l] = W[16mt + (l&15)][16*(r>>2) + 4*(l>>4) + (r&3)] */
static std::vector<float> make_frags(const HostMat &w, int &mtiles) {
    const int M = w.nc, K = w.nr;
    mtiles = (M + 15) / 16;
    const int KR = K / 4;
    std::vector<float> f((size_t)mtiles * KR * 64, 0.0f);
    for (int mt = 0; mt < mtiles; mt++)
        for (int r = 0; r < KR; r++)
            for (int l = 0; l < 64; l++) {
                const int m = 16 * mt + (l & 15);
                const int k = 16 * (r >> 2) + 4 * (l >> 4) + (r & 3);
                if (m < M) f[((size_t)mt * KR + r) * 64 + l] = w.v[(size_t)m * K + k];
            }
    return f;
}

/* fp32 -> fp16, round to nearest even (the device's v_cvt_f16_f32), and back */
static uint16_t f32_to_f16_rne(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0));       /* inf / nan */
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                          /* rounds to >= 65520: inf */
    if (x < 0x33000001u) return (uint16_t)sign;                                                       /* <= 2^-25: zero */
    if (x < 0x38800000u) {                                                                            /* subnormal half */
        const int e = (int)(x >> 23);                      /* 102 .. 112 */
        uint32_t m = (x & 0x7fffffu) | 0x800000u;
        const int shift = 126 - e;                         /* 14 .. 24: m * 2^(e - 150) in units of 2^-24 */
        const uint32_t r = m >> shift, rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
        return (uint16_t)(sign | (r + ((rem > half || (rem == half && (r & 1))) ? 1 : 0)));
    }
    const uint32_t r = x - 0x38000000u;                    /* rebias: 127 -> 15 */
    const uint32_t h = r >> 13, rem = r & 0x1fffu;
    return (uint16_t)(sign | (h + ((rem > 0x1000u || (rem == 0x1000u && (h & 1))) ? 1 : 0)));
}
static float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31, m = h & 0x3ffu;
    float f;
    if (e == 0) f = ldexpf((float)m, -24);
    else if (e == 31) f = m ? NAN : INFINITY;
    else f = ldexpf((float)(m | 0x400u), (int)e - 25);
    uint32_t x; memcpy(&x, &f, 4); x |= sign; memcpy(&f, &x, 4);
    return f;
}

/* The same rows as fp16 pieces for the split products (sh_kernels.h): 256 x = p1 + p2, cut here once.
 * piece[((mt*KS + ks)*2 + pc)*256 + l*4 + w] holds, as two halves (low = j even), the values
 * j = 2w, 2w+1 of W[16mt + (l&15)][32ks + 16(j>>2) + 4(l>>4) + (j&3)] -- the 8 values of k lane l feeds to one
 * v_mfma_f32_16x16x32_f16, in the order the activations' chunks deliver them. */
static std::vector<uint32_t> make_piece_frags(const HostMat &w) {
    const int M = w.nc, K = w.nr;
    const int mtiles = (M + 15) / 16, KS = K / 32;
    std::vector<uint32_t> f((size_t)mtiles * KS * 2 * 256, 0u);
    for (int mt = 0; mt < mtiles; mt++)
        for (int ks = 0; ks < KS; ks++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    const int m = 16 * mt + (l & 15);
                    const int k = 32 * ks + 16 * (j >> 2) + 4 * (l >> 4) + (j & 3);
                    if (m >= M) continue;
                    const float x = w.v[(size_t)m * K + k] * SH_WSCALE;
                    const uint16_t p1 = f32_to_f16_rne(x);
                    const uint16_t p2 = f32_to_f16_rne(x - f16_to_f32(p1));
                    const size_t base = ((size_t)(mt * KS + ks) * 2) * 256 + (size_t)l * 4 + (j >> 1);
                    f[base] |= (uint32_t)p1 << (16 * (j & 1));
                    f[base + 256] |= (uint32_t)p2 << (16 * (j & 1));
                }
    return f;
}
/* ... and for v_mfma_f32_32x32x16_f16 (k_gru_proj32, sh_gru32.h): m-tiles of 32 rows, k steps of 16.
 * piece[((mt*KS + ks)*2 + pc)*256 + l*4 + w]: values j = 2w, 2w+1 of W[32mt + (l&31)][16ks + 8(j>>2) + 4(l>>5) + (j&3)] -- the k order in
 * which a lane's 16 accumulator values (units 8g + 4(l>>5) + 0..3, g = 0..3) become the B operand of two k steps. */
static std::vector<uint32_t> make_piece_frags32(const HostMat &w) {
    const int M = w.nc, K = w.nr;
    const int mtiles = M / 32, KS = K / 16;
    std::vector<uint32_t> f((size_t)mtiles * KS * 2 * 256, 0u);
    for (int mt = 0; mt < mtiles; mt++)
        for (int ks = 0; ks < KS; ks++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    const int m = 32 * mt + (l & 31);
                    const int k = 16 * ks + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3);
                    const float x = w.v[(size_t)m * K + k] * SH_WSCALE;
                    const uint16_t p1 = f32_to_f16_rne(x);
                    const uint16_t p2 = f32_to_f16_rne(x - f16_to_f32(p1));
                    const size_t base = ((size_t)(mt * KS + ks) * 2) * 256 + (size_t)l * 4 + (j >> 1);
                    f[base] |= (uint32_t)p1 << (16 * (j & 1));
                    f[base + 256] |= (uint32_t)p2 << (16 * (j & 1));
                }
    return f;
}
/* bias table of k_gru_proj32, accumulator units: t[(mt*2 + hf)*16 + r] = 2^14 b[32mt + 8(r>>2) + 4hf + (r&3)] */
static std::vector<float> make_bias32(const HostMat &b) {
    const int M = b.nr * b.nc, mtiles = M / 32;
    std::vector<float> t((size_t)mtiles * 32, 0.0f);
    for (int mt = 0; mt < mtiles; mt++)
        for (int hf = 0; hf < 2; hf++)
            for (int r = 0; r < 16; r++) t[((size_t)mt * 2 + hf) * 16 + r] = b.v[32 * mt + 8 * (r >> 2) + 4 * hf + (r & 3)] * SH_OSCALE;
    return t;
}
/* operand range of the split products (sh_kernels.h): |w| * SH_WSCALE must stay a finite fp16 */
static float max_abs(const HostMat &w) {
    float m = 0.0f;
    for (float x : w.v) { const float a = std::fabs(x); if (std::isnan(a)) return a; if (a > m) m = a; }      /* a NaN anywhere is the answer */
    return m;
}
static bool in_split_range(const HostMat &w) { return max_abs(w) < SH_W_LIMIT; }

static int upload_u32(DBuf &d, const std::vector<uint32_t> &h) {
    if (d.ensure(std::max<size_t>(h.size(), 1) * 4)) return -1;
    if (!h.empty() && hipMemcpy(d.p, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return set_err("hipMemcpy of weights failed");
    return 0;
}

/* bias in accumulator (D) layout: bf[(mt*64 + l)*4 + r] = b[16mt + 4*(l>>4) + r] */
static std::vector<float> make_bias_frags(const HostMat &b, int mtiles) {
    const int M = b.nr * b.nc;
    std::vector<float> f((size_t)mtiles * 256, 0.0f);
    for (int mt = 0; mt < mtiles; mt++)
        for (int l = 0; l < 64; l++)
            for (int r = 0; r < 4; r++) {
                const int m = 16 * mt + 4 * (l >> 4) + r;
                if (m < M) f[((size_t)mt * 64 + l) * 4 + r] = b.v[m];
            }
    return f;
}

/* ... in the accumulator units of the split products (2^14) */
static std::vector<float> scaled(std::vector<float> v, float f) { for (float &x : v) x *= f; return v; }

static int upload(DBuf &d, const std::vector<float> &h) {
    if (d.ensure(h.size() * sizeof(float))) return -1;
    HIPCHK(hipMemcpy(d.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
