// smz_mlp_large.hip -- the recurrent `mlp_model` networks for up to SMZ_MAX_ACTIONS_LARGE actions in ONE launch
// (C ABI: smz_mlp_layout_large / smz_mlp_recurrent_large): H <= 128, 2 S <= 128, no limit on A + S.
//
// The wide tile kernel (smz_mlp_wide_device.hpp) holds every layer in one 128-wide pass, so its input layer takes the
// [hidden | one-hot action] row (S + A inputs) and its prediction output layer is [policy | value] (A + S <= 128 outputs).
// Here the two layers whose width grows with the action count are taken apart, everything between them is the wide kernel's
// own code (wide_layer, wide_between), compiled with the same flags:
//   * input layer.  Linear(S + A, H) on [hidden | onehot(a)] = bias + hidden . W[:S] + W[S + a].  The packed image stores the
//     hidden part (S rows padded to the 8-input groups of wide_layer, padding rows zero) followed by an action table [A][128]
//     (row a = W[S + a], plain floats).  The kernel runs wide_layer over the hidden part and adds row a of the table: no
//     [B, S + A] input buffer, no MFMA groups of zeros.  The action is range-checked: anything outside [0, A) counts as action
//     0 (a tree that is switched off leaves its last_action unwritten) and never indexes the table.
//   * prediction output layer.  ceil(A / 128) policy panels of 128 columns each (the last one ragged), then one value panel
//     (S columns); a panel is a matrix wide_layer takes as it is.  The softmax over A runs across the panels: every lane
//     writes its logits to its own places of policy_out (parked there; no LDS: 16 leaves x 1024 logits would be 64 KB per
//     wavefront and cap a CU at two of them) and keeps a running maximum and a running sum of exp(logit - maximum), rescaled
//     when the maximum moves; after the last panel the lanes of a leaf combine maximum and sum, and every lane re-reads the
//     logits IT wrote (same thread, same addresses: program order) and overwrites them with exp(logit - max) / sum.
// Two geometries (smz_mlp_recurrent_large picks by the batch size):
//   * k_mlp_recurrent_large: a wavefront per tile, all panels of a tile one after the other.  Large batches: tiles fill the chip.
//   * k_mlp_recurrent_large_split: a workgroup of four wavefronts per tile.  Each wavefront computes the trunk for itself (the
//     same bits four times: cheaper than passing it round) and takes every fourth panel; maxima and sums meet in LDS in a fixed
//     order.  Small batches have fewer tiles than the chip has SIMDs, and a round lasts as long as one tile: this makes the tile
//     shorter (at A = 1024, H = 64: 52 eight-input groups per wavefront instead of 108).
// A leaf's outputs do not depend on its tile mates.  Network outputs are held to the tolerances of the wide kernel against
// the float64 restatement (tests/test_gpu_mlp_large_heads.py), not bit parity with it: the input layer sums in another order,
// and the two geometries add the panels' sums in different orders.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"
#include "smz_mlp_wide_device.hpp"
#include "smz_mlp_large_device.hpp"          // large_tile, large_panels, r8, kLargeWaves

using namespace smz_mlp;

namespace {

constexpr int kLargeChunk = 32;              // rows per workgroup trip: at most one wavefront's lanes (the lists come from ballots)
constexpr int kLargeMaxWgs = 2048;           // grid cap; a launch of more than kLargeMaxWgs * kLargeChunk rows grid-strides
constexpr int kLargeSplitMax = 2048;         // largest batch of the split geometry at A <= 128 (2 x 128 workgroups); twice that above

// A workgroup takes chunks of kLargeChunk rows.  Every wavefront lists the chunk's rows per branch by itself (two ballots, its
// own 64 list entries in LDS: no workgroup barrier, no atomics, a fixed order) and takes every kLargeWaves-th tile.
__global__ void __launch_bounds__(kLargeWaves *kWave) k_mlp_recurrent_large(smz_mlp_desc d, const float *__restrict__ weights,
                                                                            const float *__restrict__ parent_hidden,
                                                                            const int32_t *__restrict__ last_action,
                                                                            const uint8_t *__restrict__ branch,
                                                                            float *__restrict__ hidden_out, float *__restrict__ reward_out,
                                                                            float *__restrict__ policy_out, float *__restrict__ value_out,
                                                                            int B) {
    __shared__ float4 tiles4[kLargeWaves * kWideTileFloats / 4];
    __shared__ unsigned short lists[kLargeWaves][2 * kLargeChunk];
    const int S = d.S, A = d.A;
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    float *tile = reinterpret_cast<float *>(tiles4) + wave * kWideTileFloats;
    unsigned short *list = lists[wave];
    for (int base = blockIdx.x * kLargeChunk; base < B; base += gridDim.x * kLargeChunk) {
        const int n = B - base < kLargeChunk ? B - base : kLargeChunk;
        const bool row = lane < n;
        const bool dyn = row && branch[base + (row ? lane : 0)] != 0;
        const unsigned long long m_dyn = __ballot(dyn), m_ady = __ballot(row && !dyn);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (row) list[dyn ? __popcll(m_dyn & below) : kLargeChunk + __popcll(m_ady & below)] = (unsigned short)lane;
        lds_sync();
        const int n0 = __popcll(m_dyn), n1 = __popcll(m_ady);
        const int t0 = (n0 + kTileLeaves - 1) / kTileLeaves, t1 = (n1 + kTileLeaves - 1) / kTileLeaves;
        for (int tl = wave; tl < t0 + t1; tl += kLargeWaves) {
            const bool ady = tl >= t0;                                       // wave-uniform
            const int tt = ady ? tl - t0 : tl, count = (ady ? n1 : n0) - tt * kTileLeaves;
            const unsigned short *li = list + (ady ? kLargeChunk : 0) + tt * kTileLeaves;
            large_tile<1>(d, weights, tile, count, ady, lane, 0, nullptr,
                          [&](int lf, int k) { return parent_hidden[(size_t)(base + li[lf]) * S + k]; },
                          [&](int lf) { return last_action[base + li[lf]]; },
                          [&](int lf) {
                              const int r = base + li[lf];
                              return WideDst{hidden_out + (size_t)r * S, policy_out + (size_t)r * A, value_out + r,
                                             reward_out ? reward_out + r : nullptr};
                          });
        }
        lds_sync();                                                          // the list is rewritten for the next chunk
    }
}

// Small batches: workgroup (c, b) takes the rows of branch b (blockIdx.y = 0: dynamics, 1: afterstate) among the 16 rows of
// chunk c -- at most one tile -- and its four wavefronts share the tile's panels.  Every wavefront builds the same list from the
// same ballot, so all four skip an empty tile together and meet at the same barriers.
__global__ void __launch_bounds__(kLargeWaves *kWave) k_mlp_recurrent_large_split(smz_mlp_desc d, const float *__restrict__ weights,
                                                                                  const float *__restrict__ parent_hidden,
                                                                                  const int32_t *__restrict__ last_action,
                                                                                  const uint8_t *__restrict__ branch,
                                                                                  float *__restrict__ hidden_out, float *__restrict__ reward_out,
                                                                                  float *__restrict__ policy_out, float *__restrict__ value_out,
                                                                                  int B) {
    __shared__ float4 tiles4[kLargeWaves * kWideTileFloats / 4];
    __shared__ unsigned short lists[kLargeWaves][kTileLeaves];
    __shared__ float2 xw2[kLargeWaves * kTileLeaves];
    const int S = d.S, A = d.A;
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    float *tile = reinterpret_cast<float *>(tiles4) + wave * kWideTileFloats;
    unsigned short *list = lists[wave];
    const bool ady = blockIdx.y != 0;
    for (int base = blockIdx.x * kTileLeaves; base < B; base += gridDim.x * kTileLeaves) {
        const int n = B - base < kTileLeaves ? B - base : kTileLeaves;
        const bool row = lane < n;
        const bool take = row && (branch[base + (row ? lane : 0)] != 0) != ady;
        const unsigned long long mask = __ballot(take);
        if (take) list[__popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)lane;
        lds_sync();
        const int count = __popcll(mask);
        if (count > 0)                                                       // (the same in all four wavefronts)
            large_tile<kLargeWaves>(d, weights, tile, count, ady, lane, wave, reinterpret_cast<float *>(xw2),
                                    [&](int lf, int k) { return parent_hidden[(size_t)(base + list[lf]) * S + k]; },
                                    [&](int lf) { return last_action[base + list[lf]]; },
                                    [&](int lf) {
                                        const int r = base + list[lf];
                                        return WideDst{hidden_out + (size_t)r * S, policy_out + (size_t)r * A, value_out + r,
                                                       reward_out ? reward_out + r : nullptr};
                                    });
        lds_sync();                                                          // the list is rewritten for the next chunk
    }
}

}  // namespace

extern "C" {

int smz_mlp_layout_large(smz_mlp_desc *d) {
    if (!d || d->obs < 1 || d->A < 1 || d->S < 1 || d->H < 1 || d->L < 0) return SMZ_ERR_INVALID;
    if (d->A > SMZ_MAX_ACTIONS_LARGE || d->H > kWideOP || 2 * d->S > kWideOP) return SMZ_ERR_TOO_LARGE;
    d->OP = kWideOP;
    const int mid = d->L > 0 ? r8(d->H) : 0;         // one shared Linear(H, H) per trunk, applied L times
    const int in = r8(d->S) + d->A;                  // hidden part (8-input groups) + one table row per action
    const int pan = large_panels(d->A) + 1;          // policy panels + the value panel
    const int rows[M_COUNT] = {in, in, mid, mid, r8(d->H), r8(d->H), r8(d->S), r8(d->S), mid, mid, pan * r8(d->H), pan * r8(d->H),
                               r8(d->obs), mid, r8(d->H)};
    int off = 0;
    for (int m = 0; m < M_COUNT; m++) { d->off[m] = off; off += rows[m] * kWideOP; }
    for (int m = 0; m < M_COUNT; m++) {
        d->off[M_COUNT + m] = off;
        off += (m == M_PRE_OUT || m == M_APR_OUT ? pan : 1) * kWideOP;       // one bias vector per panel
    }
    d->total_floats = off;
    return SMZ_OK;
}

int smz_mlp_recurrent_large(const smz_mlp_desc *d, const float *weights_dev, const float *parent_hidden_dev,
                            const int32_t *last_action_dev, const uint8_t *branch_dev, float *hidden_out_dev,
                            float *reward_out_dev, float *policy_out_dev, float *value_out_dev, int B, smz_stream stream) {
    if (!d || !weights_dev || !parent_hidden_dev || !last_action_dev || !branch_dev || !hidden_out_dev || !reward_out_dev ||
        !policy_out_dev || !value_out_dev || B < 1)
        return SMZ_ERR_INVALID;
    smz_mlp_desc t = *d;
    if (smz_mlp_layout_large(&t) != SMZ_OK || t.total_floats != d->total_floats || d->OP != kWideOP) return SMZ_ERR_INVALID;
    for (int m = 0; m < 2 * M_COUNT; m++)
        if (t.off[m] != d->off[m]) return SMZ_ERR_INVALID;
    // geometry of small batches: chunks of 16 rows, one workgroup of 4 wavefronts per chunk and branch (at most one tile), the
    // tile's panels shared among the wavefronts.  At B = 2048 that is 256 workgroups: a wavefront on every SIMD of the chip.  A
    // tile with two or more policy panels (A > 128) still gains from the split at 4096 rows, a tile with one loses there
    // (profiles/r13_large_heads_split_ab.txt): up to B = 4096 for A > 128, up to B = 2048 otherwise.  No grid-stride trip
    // happens (256 chunks at most); the loop in the kernel is there for a smaller grid.
    int split_max = large_panels(d->A) >= 2 ? 2 * kLargeSplitMax : kLargeSplitMax;
    if (const char *e = getenv("SMZ_MLP_LARGE_SPLIT_MAX")) split_max = atoi(e);     // (A/B runs: 0 = never split)
    if (B <= split_max) {
        hipLaunchKernelGGL(k_mlp_recurrent_large_split, dim3((B + kTileLeaves - 1) / kTileLeaves, 2), dim3(kLargeWaves * kWave), 0,
                           (hipStream_t)stream, *d, weights_dev, parent_hidden_dev, last_action_dev, branch_dev, hidden_out_dev,
                           reward_out_dev, policy_out_dev, value_out_dev, B);
        return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
    }
    // geometry from B = 2049 / 4097 on: chunks of 32 rows (one or two tiles per branch) on 4 wavefronts, a wavefront per tile.  Up to
    // kLargeMaxWgs * kLargeChunk = 65 536 rows every workgroup makes one trip; row 65 536 (B = 65 537) starts the second
    // grid-stride trip of workgroup 0 (tests/test_gpu_mlp_large_heads.py runs B = 65 553).
    int wgs = (B + kLargeChunk - 1) / kLargeChunk;
    if (wgs > kLargeMaxWgs) wgs = kLargeMaxWgs;
    hipLaunchKernelGGL(k_mlp_recurrent_large, dim3(wgs), dim3(kLargeWaves * kWave), 0, (hipStream_t)stream, *d, weights_dev,
                       parent_hidden_dev, last_action_dev, branch_dev, hidden_out_dev, reward_out_dev, policy_out_dev,
                       value_out_dev, B);
    return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
}

}  // extern "C"
