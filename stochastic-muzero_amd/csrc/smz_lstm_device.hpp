// smz_lstm_device.hpp -- device code of the `lstm_model` heads, shared by the stand-alone head kernels (smz_lstm.hip) and the
// whole-search kernel (smz_lstm_search.hip).  Both files are compiled with the same flags (-ffp-contract=off), so a row goes
// through the same instructions in the same order on either path: their searches are bit-identical
// (tests/test_gpu_lstm_search.py).
//
// A trunk is Linear(in, H) -> LSTM(H, O, L) on a length-1 sequence from zero state: per layer only the i, g and o gates are
// needed, and the input Linear is folded into layer 0 on the host, so a trunk is L small matrices of 3O columns.  Lane o holds
// LSTM unit o (O <= 64): the gate pre-activations go through a small LDS buffer so that lane o sees its i, g and o columns.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"

namespace smz_lstm {

using namespace smz_mlp;

constexpr int kWavesPerWg = 4;        // ~67 KB of trunks (CartPole shape) + 4 waves of scratch: two workgroups per CU
constexpr int kMaxUnits = 64;         // one LSTM unit per lane
enum { T_DYN_RW = 0, T_DYN_ST, T_ADY_ST, T_PRE_POL, T_PRE_VAL, T_APR_POL, T_APR_VAL };

__host__ __device__ inline int w_index(int t, int l) { return 2 * (t * SMZ_LSTM_MAX_LAYERS + l); }

// per-wave LDS scratch of one row: gate pre-activations (3 x 64) | layer output | scaled state (prediction input)
constexpr int kRowScratch = 3 * kMaxUnits + 2 * kMaxUnits;
// ... with the input row in front of it (the stand-alone kernels evaluate one row at a time)
__host__ __device__ inline int scratch_floats(int in_width) { return up4(in_width) + kRowScratch; }

__device__ inline float lstm_sigmoid(float x) { return 1.f / (1.f + smz_exp(-x)); }
// |x| >= 0.5: 1 - 2 / (e^2x + 1), which saturates to +-1 without overflow (e^2x = inf gives 1, e^2x = 0 gives -1).  Below,
// that form loses the low bits of a small result to the cancellation (13 ulp on the logits of a freshly initialised net,
// whose gate pre-activations are ~0.05), so the odd Taylor series takes over: < 1 ulp on [-0.5, 0.5] in float32.
__device__ inline float lstm_tanh(float x) {
    if (fabsf(x) >= 0.5f) return 1.f - 2.f / (smz_exp(2.f * x) + 1.f);
    const float x2 = x * x;
    float p = -443861162.f / 1856156927625.f;
    p = p * x2 + 6404582.f / 10854718875.f;
    p = p * x2 + -929569.f / 638512875.f;
    p = p * x2 + 21844.f / 6081075.f;
    p = p * x2 + -1382.f / 155925.f;
    p = p * x2 + 62.f / 2835.f;
    p = p * x2 + -17.f / 315.f;
    p = p * x2 + 2.f / 15.f;
    p = p * x2 + -1.f / 3.f;
    return x + (x * x2) * p;
}

// gbuf[c] = bias[c] + sum_k W[k][c] * in[k] for c < G (row width G, in zero-padded to K4).  Columns past G read the next
// pieces of the image (or its zero slack): finite or not, they are never stored.
template <int U>
__device__ inline void gate_columns(const float *W, const float *bias, const float *in, int K4, int G, int lane, float *gbuf) {
    const float *w[1] = {W}, *b[1] = {bias}, *a[1] = {in};
    float acc[1][U];
    dense<U, 1>(w, b, a, K4, G, lane, acc);
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int c = lane + smz_mlp::kWave * u;
        if (c < G) gbuf[c] = acc[0][u];
    }
}

// One trunk (all L layers) on the row `in` (K inputs, zero-padded to up4(K)).  Returns unit `lane`'s output of the last
// layer (0 for lane >= O); hbuf receives it too, zero-padded to up4(O).
__device__ inline float lstm_trunk(const float *img, const smz_lstm_desc &d, int t, const float *in, int K, int O,
                                   float *gbuf, float *hbuf, int lane) {
    const int G = 3 * O;
    float h = 0.f;
    for (int l = 0; l < d.L; l++) {
        const float *W = img + d.off[w_index(t, l)], *bias = img + d.off[w_index(t, l) + 1];
        const float *src = l == 0 ? in : hbuf;
        const int K4 = up4(l == 0 ? K : O);
        if (G <= smz_mlp::kWave) gate_columns<1>(W, bias, src, K4, G, lane, gbuf);
        else if (G <= 2 * smz_mlp::kWave) gate_columns<2>(W, bias, src, K4, G, lane, gbuf);
        else gate_columns<3>(W, bias, src, K4, G, lane, gbuf);
        lds_sync();
        h = 0.f;
        if (lane < O) {
            const float c = lstm_sigmoid(gbuf[lane]) * lstm_tanh(gbuf[O + lane]);
            h = lstm_sigmoid(gbuf[2 * O + lane]) * lstm_tanh(c);
        }
        if (lane < up4(O)) hbuf[lane] = h;
        lds_sync();
    }
    return h;
}

// the image's [0, n) floats to the same offsets in LDS (n and the base a multiple of 4 floats)
__device__ inline void stage(float *lds, const float *weights, int n) {
    const float4 *src = reinterpret_cast<const float4 *>(weights);
    float4 *dst = reinterpret_cast<float4 *>(lds);
    for (int i = threadIdx.x; i < n / 4; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// One row of the recurrent heads by one wavefront: xin = parent hidden row | one-hot action, zero-padded to up4(S + A), in LDS;
// `rs` = kRowScratch floats of this wave's LDS; `img` = the staged trunk image.  Only the pair of networks the branch flag
// selects runs (monte_carlo_tree_search.py:333-342).  The scaled hidden row goes to hidden_dst (S floats), the policy to
// policy_dst (A floats); reward (0 on the afterstate branch) and value are returned in every lane.
__device__ inline void recurrent_row(const float *img, const smz_lstm_desc &d, const float *xin, float *rs, bool dyn, int lane,
                                     float *hidden_dst, float *policy_dst, float &reward, float &value) {
    const int S = d.S, A = d.A, K = S + A;
    float *gbuf = rs, *hbuf = gbuf + 3 * kMaxUnits, *st = hbuf + kMaxUnits;
    if (lane >= S && lane < up4(S)) st[lane] = 0.f;
    lds_sync();
    reward = 0.f;
    float v[1];
    if (dyn) {
        v[0] = lstm_trunk(img, d, T_DYN_RW, xin, K, S, gbuf, hbuf, lane);
        reward = decode_lanes<1>(v, 0, S, lane);
        v[0] = lstm_trunk(img, d, T_DYN_ST, xin, K, S, gbuf, hbuf, lane);
    } else {
        v[0] = lstm_trunk(img, d, T_ADY_ST, xin, K, S, gbuf, hbuf, lane);
    }
    scale_lanes<1>(v, 0, S, lane, st, hidden_dst);
    lds_sync();
    v[0] = lstm_trunk(img, d, dyn ? T_PRE_POL : T_APR_POL, st, S, A, gbuf, hbuf, lane);
    softmax_lanes<1>(v, A, lane, policy_dst);
    v[0] = lstm_trunk(img, d, dyn ? T_PRE_VAL : T_APR_VAL, st, S, S, gbuf, hbuf, lane);
    value = decode_lanes<1>(v, 0, S, lane);
}

// the descriptor is what smz_lstm_layout computes for its dimensions
inline int desc_check(const smz_lstm_desc *d, const void *w) {
    if (!d || !w) return SMZ_ERR_INVALID;
    smz_lstm_desc t = *d;
    if (smz_lstm_layout(&t) != SMZ_OK || t.total_floats != d->total_floats || t.recurrent_floats != d->recurrent_floats)
        return SMZ_ERR_INVALID;
    for (int i = 0; i < SMZ_LSTM_OFFSETS; i++)
        if (t.off[i] != d->off[i]) return SMZ_ERR_INVALID;
    return SMZ_OK;
}

}  // namespace smz_lstm
