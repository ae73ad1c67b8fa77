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
#include "smz_lstm_device.hpp"

using namespace smz_mlp;
using namespace smz_lstm;      // trunks, row body and LDS scratch map: shared with the whole-search kernel (smz_lstm_search.hip)

namespace {

extern __shared__ float4 smz_lstm_lds4[];

constexpr int kLdsBytes = 160 * 1024;
constexpr int kMaxObs = 4096;

__global__ void __launch_bounds__(kWavesPerWg * 64) k_lstm_recurrent(smz_lstm_desc d, const float *weights, const float *x,
                                                                     const uint8_t *branch, float *hidden_out, float *reward_out,
                                                                     float *policy_out, float *value_out, int B,
                                                                     int rows_per_wave) {
    float *lds = reinterpret_cast<float *>(smz_lstm_lds4);
    stage(lds, weights, d.recurrent_floats);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int S = d.S, A = d.A, K = S + A;
    float *xin = lds + d.recurrent_floats + wave * scratch_floats(K);
    float *rs = xin + up4(K);
    const int row0 = (blockIdx.x * kWavesPerWg + wave) * rows_per_wave;
    for (int i = 0; i < rows_per_wave; i++) {
        const int row = row0 + i;
        if (row >= B) break;                       // wave-uniform
        for (int k = lane; k < up4(K); k += kWave) xin[k] = k < K ? x[(size_t)row * K + k] : 0.f;
        float reward, value;
        recurrent_row(lds, d, xin, rs, branch[row] != 0, lane, hidden_out + (size_t)row * S, policy_out + (size_t)row * A, reward,
                      value);
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
    if (desc_check(d, weights_dev) != SMZ_OK || !obs_dev || !hidden_out_dev || !policy_out_dev || B < 1) return SMZ_ERR_INVALID;
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
    if (desc_check(d, weights_dev) != SMZ_OK || !mlp_input_dev || !branch_dev || !hidden_out_dev || !policy_out_dev ||
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
