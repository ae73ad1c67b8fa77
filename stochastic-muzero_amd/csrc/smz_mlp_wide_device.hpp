// smz_mlp_wide_device.hpp -- device code of the wide `mlp_model` tile kernel, shared by the stand-alone head kernel
// (k_mlp_recurrent_wide, smz_mlp.hip) and the whole-search kernel (k_search_mlp_wide, smz_mlp_wide_search.hip).  Both files are
// compiled with the same flags (-ffp-contract=off) and a leaf's result does not depend on its tile mates, so a leaf goes
// through the same instructions in the same order on either path: their searches are bit-identical
// (tests/test_gpu_mlp_wide_search.py).
//
// Networks too wide for LDS residency (the reference's config/experiment_434_config.json: state_space_dimensions 61,
// hidden_layer_dimensions 126, and its checkpoint 450 with number_of_hidden_layer 4; any shape with H <= 128, 2 S <= 128,
// A + S <= 128 -- hidden layers are the same Linear(H, H) applied L times, neural_network_mlp_model.py:122-142): 16-leaf
// tiles with the weights streamed from L2 -- A operands as 8-byte global loads of a 128-wide packed image
// (smz_mlp_layout_wide), prefetched one input group ahead of the MFMAs that consume them; layers are 8 tiles of 16
// neurons, dimensions are run-time values.
// The large-action head kernels (smz_mlp_large.hip: any A up to 1024) take the same pieces -- wide_layer, wide_nets,
// wide_trunk_store, wide_between -- and replace only the two layers whose width depends on the action count.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"

namespace smz_mlp {

typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int kTileLeaves = 16;
constexpr int kWideOP = 128, kWideTiles = 8;
constexpr int kWideTileFloats = 64 * 32;              // [64 input pairs][16 leaves][2]

__device__ inline float lane_xor16(float v) {
    const unsigned u = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return __uint_as_float(((threadIdx.x & 16) ? r[0] : r[1]));
}
__device__ inline float lane_xor32(float v) {
    const unsigned u = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(((threadIdx.x & 32) ? r[0] : r[1]));
}
__device__ inline float tile_max(float m) { m = fmaxf(m, lane_xor16(m)); return fmaxf(m, lane_xor32(m)); }
__device__ inline float tile_min(float m) { m = fminf(m, lane_xor16(m)); return fminf(m, lane_xor32(m)); }

__device__ inline void wide_layer(const float *__restrict__ W, const float *__restrict__ bias, const float *xp, int K8, int lane, v4f (&y)[kWideTiles]) {
    const int g = lane >> 4, j = lane & 15;
    v4f o[kWideTiles];                                      // y = the even-input accumulators (from the bias), o = the odd ones
    float2 wa[3][kWideTiles];                               // weights of three consecutive input groups: two in flight ahead
    const float *Wl = W + ((size_t)(g >> 1) * kWideOP + j) * 4 + 2 * (g & 1);
    auto wload = [&](int slot, int c) {
#pragma unroll
        for (int t = 0; t < kWideTiles; t++) wa[slot][t] = *reinterpret_cast<const float2 *>(Wl + ((size_t)2 * c * kWideOP + 16 * t) * 4);
    };
#pragma unroll
    for (int t = 0; t < kWideTiles; t++) {
        const float4 b = *reinterpret_cast<const float4 *>(bias + 16 * t + 4 * g);
        y[t] = v4f{b.x, b.y, b.z, b.w};
        o[t] = v4f{0.f, 0.f, 0.f, 0.f};
    }
    wload(0, 0);
    if (K8 > 1) wload(1, 1);
    for (int c = 0; c < K8; c += 3) {                       // three input groups per trip: static indices into wa[]
#pragma unroll
        for (int h = 0; h < 3; h++) {
            const int cc = c + h;
            if (cc < K8) {                                  // wave-uniform
                const float2 xb = *reinterpret_cast<const float2 *>(xp + ((4 * cc + g) * kTileLeaves + j) * 2);
                if (cc + 2 < K8) wload((h + 2) % 3, cc + 2);
#pragma unroll
                for (int t = 0; t < kWideTiles; t++) {
                    y[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[h][t].x, xb.x, y[t], 0, 0, 0);
                    o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[h][t].y, xb.y, o[t], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kWideTiles; t++) y[t] = y[t] + o[t];
}
__device__ inline float wide_sum(float s) { s = s + lane_xor16(s); return s + lane_xor32(s); }

// where the results of one leaf go: the new hidden row (S floats), the policy (A floats), value and reward (reward: may be null)
struct WideDst {
    float *hidden, *policy, *value, *reward;
};

// the matrices and biases of one branch's pair of networks (ady: afterstate dynamics + afterstate prediction)
// (selects between constant-index descriptor entries: a run-time index would put the table in scratch)
struct WideNets {
    int w_in, b_in, w_mid, b_mid, w_out, b_out, wp_in, bp_in, wp_mid, bp_mid, wp_out, bp_out;
};
__device__ inline WideNets wide_nets(const smz_mlp_desc &d, bool ady) {
    WideNets n;
    n.w_in = ady ? d.off[M_ADY_IN] : d.off[M_DYN_IN]; n.b_in = ady ? d.off[M_COUNT + M_ADY_IN] : d.off[M_COUNT + M_DYN_IN];
    n.w_out = ady ? d.off[M_ADY_OUT] : d.off[M_DYN_OUT]; n.b_out = ady ? d.off[M_COUNT + M_ADY_OUT] : d.off[M_COUNT + M_DYN_OUT];
    n.wp_in = ady ? d.off[M_APR_IN] : d.off[M_PRE_IN]; n.bp_in = ady ? d.off[M_COUNT + M_APR_IN] : d.off[M_COUNT + M_PRE_IN];
    n.wp_out = ady ? d.off[M_APR_OUT] : d.off[M_PRE_OUT]; n.bp_out = ady ? d.off[M_COUNT + M_APR_OUT] : d.off[M_COUNT + M_PRE_OUT];
    n.w_mid = ady ? d.off[M_ADY_MID] : d.off[M_DYN_MID]; n.b_mid = ady ? d.off[M_COUNT + M_ADY_MID] : d.off[M_COUNT + M_DYN_MID];
    n.wp_mid = ady ? d.off[M_APR_MID] : d.off[M_PRE_MID]; n.bp_mid = ady ? d.off[M_COUNT + M_APR_MID] : d.off[M_COUNT + M_PRE_MID];
    return n;
}

// ELU of a trunk layer's outputs into the tile (neuron n = input n of the next layer)
__device__ inline void wide_trunk_store(float *tile, const v4f (&y)[kWideTiles], int lane) {
    const int g = lane >> 4, j = lane & 15;
#pragma unroll
    for (int t = 0; t < kWideTiles; t++) {
        const int nn = 16 * t + 4 * g;
        *reinterpret_cast<float2 *>(tile + (((nn >> 1) + 0) * kTileLeaves + j) * 2) = make_float2(elu(y[t][0]), elu(y[t][1]));
        *reinterpret_cast<float2 *>(tile + (((nn >> 1) + 1) * kTileLeaves + j) * 2) = make_float2(elu(y[t][2]), elu(y[t][3]));
    }
}

// Everything between the two layers whose width depends on the action count.  In: y = the sums of the dynamics input layer
// (its inputs in the tile are dead).  The dynamics trunk, its output layer, scale_to_bound_action and the reward decode, the
// prediction input layer and trunk.  Out: the prediction trunk in the tile (the inputs of the prediction output layer), the
// scaled hidden row stored to `hidden` (mine: this lane's leaf exists), the decoded reward returned (0 on the afterstate branch).
__device__ inline float wide_between(const smz_mlp_desc &d, const float *__restrict__ weights, const WideNets &n, float *tile, bool ady,
                                     int lane, bool mine, float *hidden, v4f (&y)[kWideTiles]) {
    const int S = d.S, H = d.H, half = S / 2;
    const int K8h = (H + 7) >> 3, K8s = (S + 7) >> 3;
    const int g = lane >> 4, j = lane & 15;
    lds_sync();
    wide_trunk_store(tile, y, lane);
    lds_sync();
    for (int l = 0; l < d.L; l++) {          // the SAME Linear(H, H) + ELU applied L times (neural_network_mlp_model.py:122-142)
        wide_layer(weights + n.w_mid, weights + n.b_mid, tile, K8h, lane, y);
        lds_sync();
        wide_trunk_store(tile, y, lane);
        lds_sync();
    }
    wide_layer(weights + n.w_out, weights + n.b_out, tile, K8h, lane, y);
    float reward = 0.f;
    {   // dynamics: [reward logits 0..S-1 | next state S..2S-1]; afterstate dynamics: next state 0..S-1
        const int lo = ady ? 0 : S;
        float mr = -__builtin_inff(), mn = __builtin_inff(), mx = -__builtin_inff();
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r;
                if (!ady && o < S) mr = fmaxf(mr, y[t][r]);
                if (o >= lo && o < lo + S) { mn = fminf(mn, y[t][r]); mx = fmaxf(mx, y[t][r]); }
            }
        mn = tile_min(mn); mx = tile_max(mx);
        if (!ady) {
            mr = tile_max(mr);
            float den = 0.f, num = 0.f;
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r;
                    if (o < S) { const float ev = smz_exp(y[t][r] - mr); den += ev; num += (float)(o - half) * ev; }
                }
            reward = support_to_scalar(wide_sum(num), wide_sum(den));
        }
        float sc = mx - mn;
        if (sc < 1e-5f) sc += 1e-5f;
        lds_sync();
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r, k = o - lo;
                if (k >= 0 && k < S) {
                    const float hv = __fdividef(y[t][r] - mn, sc);
                    tile[((k >> 1) * kTileLeaves + j) * 2 + (k & 1)] = hv;
                    if (mine) hidden[k] = hv;
                }
            }
        for (int i = lane; i < kTileLeaves * (8 * K8s - S); i += kWave) {          // zero inputs S .. 8 K8s - 1
            const int lf = i / (8 * K8s - S), k = S + i % (8 * K8s - S);
            tile[((k >> 1) * kTileLeaves + lf) * 2 + (k & 1)] = 0.f;
        }
    }
    lds_sync();
    wide_layer(weights + n.wp_in, weights + n.bp_in, tile, K8s, lane, y);
    lds_sync();
    wide_trunk_store(tile, y, lane);
    lds_sync();
    for (int l = 0; l < d.L; l++) {
        wide_layer(weights + n.wp_mid, weights + n.bp_mid, tile, K8h, lane, y);
        lds_sync();
        wide_trunk_store(tile, y, lane);
        lds_sync();
    }
    return reward;
}

// ONE tile of up to 16 leaves of one branch (ady: the afterstate pair of networks), by one wavefront.
//   tile     the wavefront's kWideTileFloats of LDS
//   count    leaves in the tile (>= 1; may exceed 16: the tile then takes the first 16)
//   in       in(lf, k): input k < S + A of leaf lf < min(count, 16) -- [hidden row | one-hot action]
//   dst      dst(lf): the destinations of leaf lf < min(count, 16)
// A ragged tile repeats its first leaf in the unused columns; nothing is stored for them.
template <class In, class Dst>
__device__ inline void wide_tile(const smz_mlp_desc &d, const float *__restrict__ weights, float *tile, int count, bool ady, int lane,
                                 In in, Dst dst) {
    const int S = d.S, A = d.A, H = d.H, half = S / 2, XW = S + A;
    const int K8x = (XW + 7) >> 3, K8h = (H + 7) >> 3;
    const int g = lane >> 4, j = lane & 15;
    const bool mine = j < count;
    const WideDst out = dst(mine ? j : 0);
    // network inputs [hidden | one-hot] -> tile, zero beyond them up to the layer's 8-input groups
    for (int i = lane; i < kTileLeaves * 8 * K8x; i += kWave) {
        const int lf = i / (8 * K8x), k = i % (8 * K8x);
        tile[((k >> 1) * kTileLeaves + lf) * 2 + (k & 1)] = k < XW ? in(lf < count ? lf : 0, k) : 0.f;
    }
    lds_sync();
    const WideNets n = wide_nets(d, ady);
    v4f y[kWideTiles];
    wide_layer(weights + n.w_in, weights + n.b_in, tile, K8x, lane, y);
    const float reward = wide_between(d, weights, n, tile, ady, lane, mine, out.hidden, y);
    wide_layer(weights + n.wp_out, weights + n.bp_out, tile, K8h, lane, y);
    {   // [policy logits 0..A-1 | value logits A..A+S-1]
        float mp = -__builtin_inff(), mv = -__builtin_inff();
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r;
                if (o < A) mp = fmaxf(mp, y[t][r]);
                else if (o < A + S) mv = fmaxf(mv, y[t][r]);
            }
        mp = tile_max(mp); mv = tile_max(mv);
        float dp = 0.f, dv = 0.f, nv = 0.f;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r;
                if (o < A) { y[t][r] = smz_exp(y[t][r] - mp); dp += y[t][r]; }
                else if (o < A + S) { const float ev = smz_exp(y[t][r] - mv); dv += ev; nv += (float)(o - A - half) * ev; }
            }
        dp = wide_sum(dp);
        const float value = support_to_scalar(wide_sum(nv), wide_sum(dv));
        if (mine) {
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r;
                    if (o < A) out.policy[o] = __fdividef(y[t][r], dp);
                }
            if (g == 0) {
                *out.value = value;
                if (out.reward) *out.reward = reward;
            }
        }
    }
    lds_sync();
}

}  // namespace smz_mlp
