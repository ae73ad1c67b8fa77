// smz_lstm.hip -- fused `lstm_model` head kernels (C ABI: smz_lstm_layout / _initial / _recurrent; include/smz.h).
//
// Each head of the family is Linear(in, H) -> LSTM(H, O, L) -> output sequence, called by the reference with batch 1: a
// length-1 sequence from zero state.  Per layer only the i, g and o gates are needed (f multiplies c0 = 0, W_hh multiplies
// h0 = 0), and the input Linear is folded into layer 0 on the host, so a trunk is L small matrices of 3O columns.  The seven
// recurrent trunks are staged once per workgroup in LDS; a wavefront evaluates its rows one after another, each row only the
// pair of networks its branch flag selects (monte_carlo_tree_search.py:333-342).  Lane o holds LSTM unit o (O <= 64): the
// gate pre-activations go through a small LDS buffer so that lane o sees its i, g and o columns.  Softmax, support decode and
// min-max scaling are the mlp heads' helpers.  Network outputs are held to the 1e-5 class, not bit parity.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"

using namespace smz_mlp;

namespace {

extern __shared__ float4 smz_lstm_lds4[];

constexpr int kLdsBytes = 160 * 1024;
constexpr int kWavesPerWg = 4;        // ~67 KB of trunks (CartPole shape) + 4 waves of scratch: two workgroups per CU
constexpr int kMaxUnits = 64;         // one LSTM unit per lane
constexpr int kMaxObs = 4096;
enum { T_DYN_RW = 0, T_DYN_ST, T_ADY_ST, T_PRE_POL, T_PRE_VAL, T_APR_POL, T_APR_VAL };

__host__ __device__ inline int w_index(int t, int l) { return 2 * (t * SMZ_LSTM_MAX_LAYERS + l); }

// per-wave LDS scratch: input row | gate pre-activations (3 x 64) | layer output | scaled state (prediction input)
__host__ __device__ inline int scratch_floats(int in_width) { return up4(in_width) + 3 * kMaxUnits + 2 * kMaxUnits; }

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
        const int c = lane + kWave * u;
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
        if (G <= kWave) gate_columns<1>(W, bias, src, K4, G, lane, gbuf);
        else if (G <= 2 * kWave) gate_columns<2>(W, bias, src, K4, G, lane, gbuf);
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

__global__ void __launch_bounds__(kWavesPerWg * 64) k_lstm_recurrent(smz_lstm_desc d, const float *weights, const float *x,
                                                                     const uint8_t *branch, float *hidden_out, float *reward_out,
                                                                     float *policy_out, float *value_out, int B,
                                                                     int rows_per_wave) {
    float *lds = reinterpret_cast<float *>(smz_lstm_lds4);
    stage(lds, weights, d.recurrent_floats);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int S = d.S, A = d.A, K = S + A;
    float *xin = lds + d.recurrent_floats + wave * scratch_floats(K);
    float *gbuf = xin + up4(K), *hbuf = gbuf + 3 * kMaxUnits, *st = hbuf + kMaxUnits;
    const int row0 = (blockIdx.x * kWavesPerWg + wave) * rows_per_wave;
    for (int i = 0; i < rows_per_wave; i++) {
        const int row = row0 + i;
        if (row >= B) break;                       // wave-uniform
        for (int k = lane; k < up4(K); k += kWave) xin[k] = k < K ? x[(size_t)row * K + k] : 0.f;
        if (lane >= S && lane < up4(S)) st[lane] = 0.f;
        lds_sync();
        const bool dyn = branch[row] != 0;
        float reward = 0.f;
        float v[1];
        if (dyn) {
            v[0] = lstm_trunk(lds, d, T_DYN_RW, xin, K, S, gbuf, hbuf, lane);
            reward = decode_lanes<1>(v, 0, S, lane);
            v[0] = lstm_trunk(lds, d, T_DYN_ST, xin, K, S, gbuf, hbuf, lane);
        } else {
            v[0] = lstm_trunk(lds, d, T_ADY_ST, xin, K, S, gbuf, hbuf, lane);
        }
        scale_lanes<1>(v, 0, S, lane, st, hidden_out + (size_t)row * S);
        lds_sync();
        v[0] = lstm_trunk(lds, d, dyn ? T_PRE_POL : T_APR_POL, st, S, A, gbuf, hbuf, lane);
        softmax_lanes<1>(v, A, lane, policy_out + (size_t)row * A);
        v[0] = lstm_trunk(lds, d, dyn ? T_PRE_VAL : T_APR_VAL, st, S, S, gbuf, hbuf, lane);
        const float value = decode_lanes<1>(v, 0, S, lane);
        if (lane == 0) {
            if (reward_out) reward_out[row] = reward;
            value_out[row] = value;
        }
    }
}

// representation + root policy; weights read from global memory (once per search, the trunk image stays unstaged)
__global__ void __launch_bounds__(kWavesPerWg * 64) k_lstm_initial(smz_lstm_desc d, const float *weights, const float *obs,
                                                                   float *hidden_out, float *policy_out, int B,
                                                                   int rows_per_wave) {
    float *lds = reinterpret_cast<float *>(smz_lstm_lds4);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int S = d.S, A = d.A, K = d.obs;
    float *xin = lds + wave * scratch_floats(K);
    float *gbuf = xin + up4(K), *hbuf = gbuf + 3 * kMaxUnits, *st = hbuf + kMaxUnits;
    const int row0 = (blockIdx.x * kWavesPerWg + wave) * rows_per_wave;
    for (int i = 0; i < rows_per_wave; i++) {
        const int row = row0 + i;
        if (row >= B) break;
        for (int k = lane; k < up4(K); k += kWave) xin[k] = k < K ? obs[(size_t)row * K + k] : 0.f;
        if (lane >= S && lane < up4(S)) st[lane] = 0.f;
        lds_sync();
        float v[1];
        {
            const float *w[1] = {weights + d.off[SMZ_LSTM_REP]}, *b[1] = {weights + d.off[SMZ_LSTM_REP + 1]}, *a[1] = {xin};
            float acc[1][1];
            dense<1, 1>(w, b, a, up4(K), S, lane, acc);
            v[0] = acc[0][0];
        }
        scale_lanes<1>(v, 0, S, lane, st, hidden_out + (size_t)row * S);
        lds_sync();
        v[0] = lstm_trunk(weights, d, T_PRE_POL, st, S, A, gbuf, hbuf, lane);
        softmax_lanes<1>(v, A, lane, policy_out + (size_t)row * A);
    }
}

template <typename Kern>
int allow_lds(Kern kern, size_t bytes) {
    // dynamic LDS above 64 KB needs the kernel's opt-in (a host-side runtime call, made once per kernel and size)
    static size_t granted[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return SMZ_ERR_HIP;
    if (bytes <= granted[dev]) return SMZ_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)bytes) != hipSuccess)
        return SMZ_ERR_HIP;
    granted[dev] = bytes;
    return SMZ_OK;
}

int lstm_check(const smz_lstm_desc *d, const void *w) {
    if (!d || !w) return SMZ_ERR_INVALID;
    smz_lstm_desc t = *d;
    if (smz_lstm_layout(&t) != SMZ_OK || t.total_floats != d->total_floats || t.recurrent_floats != d->recurrent_floats)
        return SMZ_ERR_INVALID;
    for (int i = 0; i < SMZ_LSTM_OFFSETS; i++)
        if (t.off[i] != d->off[i]) return SMZ_ERR_INVALID;
    return SMZ_OK;
}

void lstm_geometry(int B, int &blocks, int &rows_per_wave) {
    // two workgroups per CU (256 CUs); rows spread evenly over them
    const int waves = 512 * kWavesPerWg;
    rows_per_wave = (B + waves - 1) / waves;
    if (rows_per_wave < 1) rows_per_wave = 1;
    const int rows_per_block = rows_per_wave * kWavesPerWg;
    blocks = (B + rows_per_block - 1) / rows_per_block;
}

}  // namespace

extern "C" {

int smz_lstm_layout(smz_lstm_desc *d) {
    if (!d || d->obs < 1 || d->obs > kMaxObs || d->A < 1 || d->A > kMaxUnits || d->S < 1 || d->S > kMaxUnits || d->L < 1 ||
        d->L > SMZ_LSTM_MAX_LAYERS)
        return SMZ_ERR_INVALID;
    const int S = d->S, A = d->A;
    const int in[SMZ_LSTM_TRUNKS] = {S + A, S + A, S + A, S, S, S, S};
    const int out[SMZ_LSTM_TRUNKS] = {S, S, S, A, S, A, S};
    for (int i = 0; i < SMZ_LSTM_OFFSETS; i++) d->off[i] = 0;
    int off = 0;
    for (int t = 0; t < SMZ_LSTM_TRUNKS; t++) {
        for (int l = 0; l < d->L; l++) {
            const int K = l == 0 ? in[t] : out[t], G = 3 * out[t];
            d->off[w_index(t, l)] = off;
            off += up4(K) * G;
            d->off[w_index(t, l) + 1] = off;
            off += up4(G);
        }
    }
    off += SMZ_LSTM_SLACK;
    d->recurrent_floats = off;
    d->off[SMZ_LSTM_REP] = off;
    off += up4(d->obs) * S;
    d->off[SMZ_LSTM_REP + 1] = off;
    off += up4(S) + SMZ_LSTM_SLACK;
    d->total_floats = off;
    const size_t need = ((size_t)d->recurrent_floats + (size_t)kWavesPerWg * scratch_floats(S + A)) * sizeof(float);
    d->lds_bytes = (int)need;
    return need <= (size_t)kLdsBytes ? SMZ_OK : SMZ_ERR_INVALID;
}

int smz_lstm_initial(const smz_lstm_desc *d, const float *weights_dev, const float *obs_dev, float *hidden_out_dev,
                     float *policy_out_dev, int B, smz_stream stream) {
    if (lstm_check(d, weights_dev) != SMZ_OK || !obs_dev || !hidden_out_dev || !policy_out_dev || B < 1) return SMZ_ERR_INVALID;
    int blocks, rpw;
    lstm_geometry(B, blocks, rpw);
    const size_t lds = (size_t)kWavesPerWg * scratch_floats(d->obs) * sizeof(float);
    if (allow_lds(k_lstm_initial, lds) != SMZ_OK) return SMZ_ERR_HIP;
    hipLaunchKernelGGL(k_lstm_initial, dim3(blocks), dim3(kWavesPerWg * kWave), lds, (hipStream_t)stream, *d, weights_dev,
                       obs_dev, hidden_out_dev, policy_out_dev, B, rpw);
    return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
}

int smz_lstm_recurrent(const smz_lstm_desc *d, const float *weights_dev, const float *mlp_input_dev,
                       const uint8_t *branch_dev, float *hidden_out_dev, float *reward_out_dev, float *policy_out_dev,
                       float *value_out_dev, int B, smz_stream stream) {
    if (lstm_check(d, weights_dev) != SMZ_OK || !mlp_input_dev || !branch_dev || !hidden_out_dev || !policy_out_dev ||
        !value_out_dev || B < 1)
        return SMZ_ERR_INVALID;
    int blocks, rpw;
    lstm_geometry(B, blocks, rpw);
    const size_t lds = (size_t)d->lds_bytes;
    if (allow_lds(k_lstm_recurrent, lds) != SMZ_OK) return SMZ_ERR_HIP;
    hipLaunchKernelGGL(k_lstm_recurrent, dim3(blocks), dim3(kWavesPerWg * kWave), lds, (hipStream_t)stream, *d, weights_dev,
                       mlp_input_dev, branch_dev, hidden_out_dev, reward_out_dev, policy_out_dev, value_out_dev, B, rpw);
    return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
}

}  // extern "C"
