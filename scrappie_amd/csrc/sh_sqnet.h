/* sh_sqnet.h -- the sequence -> squiggle network (networks.c:397-565) as one fused kernel, k_sqnet.
 *
 *   embedding 4 -> 3 | conv1 3 -> 32, tanh | conv2..5 32 -> 32, tanh, + input | conv6 32 -> 3, linear
 *   every convolution: window WL (7 or 9), stride 1, zero padding of (WL - 1) / 2 columns at both sequence ends (layers.c:159-246)
 *
 * A workgroup owns SH_SQN_TP output positions of one sequence.  It works on a block of WD = TP + 2 H positions, H = 6 (WL - 1) / 2
 * being what six layers' windows reach to either side, one thread per position; the activations of the block ping-pong between two
 * LDS buffers of 32 rows (features) x SH_SQN_RS columns, and only the three output floats of the TP middle positions go to memory.
 * A layer's output at a block position outside [0, n) is stored as zero, not as what the layer computes there: that is the
 * reference's zero padding of every layer's input.  Block positions inside the sequence are computed as anywhere else; the outer
 * (WL - 1) / 2 columns lose their meaning with every layer (their windows reach outside the block, into the zero columns), which is
 * why the block carries H of them per side.  A position's value therefore depends on the sequence alone, never on the tile.
 *
 * Arithmetic: fp32 FMA on the vector ALU, bias first, then tap by tap and feature by feature (`acc = fma(w, x, acc)`), so every
 * tile and every launch sums in one order.  A thread keeps one position's 32 filters in registers; the weight of a (tap, feature,
 * filter) is the same for the whole wave, so the weights are read through the scalar cache from a table laid out [tap][feature]
 * [filter] and never touch LDS; the activation of a (feature, position + tap) is one LDS read per 32 FMAs, consecutive lanes on
 * consecutive banks.
 *
 * LDS: 2 x 32 x 256 x 4 = 64 KB (static), two workgroups per CU.  Columns [0, PAD) and [PAD + WD, RS) of every row stay zero, so
 * the taps need no bounds check. */
#pragma once

#define SH_SQN_TP 200          /* output positions per workgroup */
#define SH_SQN_NTH 256         /* threads per workgroup: one per block position */
#define SH_SQN_RS 256          /* columns per LDS row: PAD + WD + PAD <= RS for WL 7 and 9 */
#define SH_SQN_NF 32           /* filters of conv1 .. conv5 */
#define SH_SQN_NE 3            /* embedding features */
#define SH_SQN_NO 3            /* outputs: mean, log sd, dwell logit */

/* the weight table (floats): embedding [4][3] padded to 16 | conv1 W [WL][3][32], b [32] | conv2..5 W [WL][32][32], b [32] | conv6 W [WL][32][4], b [4] */
__host__ __device__ constexpr int sqn_off_c1(int) { return 16; }
__host__ __device__ constexpr int sqn_off_res(int WL, int l) { return 16 + WL * SH_SQN_NE * SH_SQN_NF + SH_SQN_NF + l * (WL * SH_SQN_NF * SH_SQN_NF + SH_SQN_NF); }
__host__ __device__ constexpr int sqn_off_c6(int WL) { return sqn_off_res(WL, 4); }
__host__ __device__ constexpr int sqn_table_floats(int WL) { return sqn_off_c6(WL) + WL * SH_SQN_NF * 4 + 4; }

struct ShSqnetTile { long long off; int n, t0; };      /* where the sequence starts in the codes / the output, its length, the tile's first output position */

struct ShSqnetArgs {
    const ShSqnetTile *tile;
    const unsigned char *code;     /* bases 0..3, sequences end to end */
    const float *w;                /* the weight table */
    float *out;                    /* [position][3], sequences end to end */
};

/* one layer for one block position: COUT filters over CIN features x WL taps; W [tap][feature][COUT], b [COUT] */
template <int WL, int CIN, bool RESID>
__device__ __forceinline__ void sqn_layer(const float *in, float *out, const float *__restrict__ W, const float *__restrict__ b, int j, bool live) {
    constexpr int PAD = (WL - 1) / 2;
    float acc[SH_SQN_NF];
#pragma unroll
    for (int f = 0; f < SH_SQN_NF; f++) acc[f] = b[f];
    for (int t = 0; t < WL; t++) {
#pragma unroll 2
        for (int c = 0; c < CIN; c++) {
            const float x = in[c * SH_SQN_RS + j + t];
            const float *wp = W + (t * CIN + c) * SH_SQN_NF;
#pragma unroll
            for (int f = 0; f < SH_SQN_NF; f++) acc[f] = __builtin_fmaf(wp[f], x, acc[f]);
        }
    }
#pragma unroll
    for (int f = 0; f < SH_SQN_NF; f++) {
        float v = d_tanh(acc[f]);
        if (RESID) v += in[f * SH_SQN_RS + PAD + j];
        out[f * SH_SQN_RS + PAD + j] = live ? v : 0.0f;
    }
}

template <int WL>
__global__ __launch_bounds__(SH_SQN_NTH) void k_sqnet(ShSqnetArgs a) {
    constexpr int PAD = (WL - 1) / 2, H = 6 * PAD, WD = SH_SQN_TP + 2 * H;
    static_assert(WD + 2 * PAD <= SH_SQN_RS && WD <= SH_SQN_NTH, "the block does not fit its LDS rows");
    __shared__ float buf[2][SH_SQN_NF * SH_SQN_RS];
    const ShSqnetTile tl = a.tile[blockIdx.x];
    const int j = (int)threadIdx.x;
    const int g = tl.t0 - H + j;                       /* the position in the sequence */
    const bool act = j < WD;
    const bool live = act && g >= 0 && g < tl.n;
    for (int i = j; i < 2 * SH_SQN_NF * SH_SQN_RS; i += SH_SQN_NTH) (&buf[0][0])[i] = 0.0f;
    __syncthreads();
    if (live) {
        const int code = a.code[tl.off + g];
#pragma unroll
        for (int c = 0; c < SH_SQN_NE; c++) buf[0][c * SH_SQN_RS + PAD + j] = a.w[code * SH_SQN_NE + c];
    }
    __syncthreads();
    if (act) sqn_layer<WL, SH_SQN_NE, false>(buf[0], buf[1], a.w + sqn_off_c1(WL), a.w + sqn_off_c1(WL) + WL * SH_SQN_NE * SH_SQN_NF, j, live);
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < 4; l++) {
        const float *W = a.w + sqn_off_res(WL, l);
        if (act) sqn_layer<WL, SH_SQN_NF, true>(buf[(l + 1) & 1], buf[l & 1], W, W + WL * SH_SQN_NF * SH_SQN_NF, j, live);
        __syncthreads();
    }
    /* conv6, linear: the tile's own positions only (after four residual layers the activations are in buf[1]) */
    if (j >= H && j < H + SH_SQN_TP && g < tl.n) {
        const float *W = a.w + sqn_off_c6(WL), *b = W + WL * SH_SQN_NF * 4;
        const float *in = buf[1];
        float acc[SH_SQN_NO];
#pragma unroll
        for (int k = 0; k < SH_SQN_NO; k++) acc[k] = b[k];
        for (int t = 0; t < WL; t++) {
#pragma unroll 4
            for (int c = 0; c < SH_SQN_NF; c++) {
                const float x = in[c * SH_SQN_RS + j + t];
                const float *wp = W + (t * SH_SQN_NF + c) * 4;
#pragma unroll
                for (int k = 0; k < SH_SQN_NO; k++) acc[k] = __builtin_fmaf(wp[k], x, acc[k]);
            }
        }
        float *o = a.out + (tl.off + g) * SH_SQN_NO;
#pragma unroll
        for (int k = 0; k < SH_SQN_NO; k++) o[k] = acc[k];
    }
}
