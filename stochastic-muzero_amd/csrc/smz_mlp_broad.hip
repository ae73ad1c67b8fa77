// smz_mlp_broad.hip -- the recurrent `mlp_model` networks up to 512 wide in ONE launch per simulation round
// (C ABI: smz_mlp_layout_broad / smz_mlp_recurrent_broad): 1 <= H <= 512, 1 <= S <= 256, 1 <= A <= SMZ_MAX_ACTIONS_LARGE.
//
// The wide and the large-action tile kernels hold a layer's outputs in one 128-wide pass of wide_layer, so they stop at
// H <= 128 and 2 S <= 128.  Here every layer is a sequence of 128-column panels (smz_mlp_broad_device.hpp):
//
// The packed image (smz_mlp_layout_broad; OP = 128, R8(x) = x rounded up to a multiple of 8, P(n) = ceil(n / 128)).  A "panel
// matrix" of K inputs and O outputs at base, with its biases at bias, is P(O) panels, panel p a wide matrix of R8(K) x 128
// floats that holds output columns 128 p .. min(O, 128 p + 128) - 1:
//     weight (k, o)  at  base + (o / 128) * R8(K) * 128 + ((k / 4) * 128 + o % 128) * 4 + k % 4
//     bias o         at  bias + o                                   (P(O) vectors of 128 floats, one per panel)
// padding rows, padding columns and padding biases are zero.  Matrices (off[] index; biases at off[15 + index]):
//     0 dyn_in, 1 ady_in     the hidden part, a panel matrix of K = S, O = H, then the action table [A][128 P(H)]:
//                            element (a, o) at off + P(H) * R8(S) * 128 + a * 128 * P(H) + o = weight of input S + a for neuron o
//     2 dyn_mid, 3 ady_mid, 8 pre_mid, 9 apr_mid, 13 rep_mid     panel matrices of K = H, O = H (absent when L = 0)
//     4 dyn_out              TWO panel matrices of K = H, O = S one after the other: the reward logits (torch rows 0 .. S - 1),
//                            then the next state (rows S .. 2 S - 1) at off + P(S) * R8(H) * 128, biases at off[15 + 4] + 128 P(S):
//                            each column range in panels of its own
//     5 ady_out, 14 rep_out  panel matrices of K = H, O = S
//     6 pre_in, 7 apr_in     panel matrices of K = S, O = H;  12 rep_in: K = obs, O = H
//     10 pre_out, 11 apr_out the policy, a panel matrix of K = H, O = A, then the value, one of K = H, O = S, at
//                            off + P(A) * R8(H) * 128, biases at off[15 + index] + 128 P(A)
// The representation matrices are packed in the same form; nothing here reads them (a root kernel would).
//
// Geometry: workgroup (c, b) of four wavefronts takes the rows of branch b (blockIdx.y = 0: dynamics, 1: afterstate) among the
// rows of chunk c, listed from a ballot.  A workgroup without a row of its branch leaves as a whole before the first barrier.
// Every 16-row tile streams the whole weight image of its branch from L2, and a round lasts as long as the longest workgroup:
//   * B <= 4096: chunks of 16 rows, at most ONE tile per workgroup (twice the workgroups, half-filled tiles on mixed branches);
//   * above: chunks of 32 rows, one or two tiles of 16 one after the other (about 1.3 tiles per 16 rows instead of 2).
// Measured (profiles/r16_broad_heads_chunk_ab.txt): 16-row chunks take 0.57x the time at 256 and 1024 trees and 0.83-0.89x at
// 4096; from 8192 trees on, where the chip is full either way, 32-row chunks take 0.79-0.86x.  A row's bits are the same in both.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"
#include "smz_mlp_wide_device.hpp"
#include "smz_mlp_broad_device.hpp"

using namespace smz_mlp;

namespace {

constexpr int kBroadChunk = 2 * kTileLeaves;     // most rows per workgroup: at most one wavefront's lanes (the list comes from a ballot)

constexpr int kBroadSmallMax = 4096;             // largest batch in chunks of 16 rows (smz_mlp_recurrent_broad)

// CH = rows per chunk: kBroadChunk (one or two tiles per workgroup) or kTileLeaves (one)
template <int CH>
__global__ void __launch_bounds__(kBroadWaves *kWave) k_mlp_recurrent_broad(smz_mlp_desc d, const float *__restrict__ weights,
                                                                            const float *__restrict__ parent_hidden,
                                                                            const int32_t *__restrict__ last_action,
                                                                            const uint8_t *__restrict__ branch,
                                                                            float *__restrict__ hidden_out, float *__restrict__ reward_out,
                                                                            float *__restrict__ policy_out, float *__restrict__ value_out,
                                                                            int B) {
    extern __shared__ float4 broad_tiles[];              // 2 x broad_tile_floats(S, H) floats
    __shared__ BroadLds lds;
    float *t0 = reinterpret_cast<float *>(broad_tiles), *t1 = t0 + broad_tile_floats(d.S, d.H);
    const int S = d.S, A = d.A;
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const bool ady = blockIdx.y != 0;
    const size_t base = (size_t)blockIdx.x * CH;
    const int n = (size_t)B - base < (size_t)CH ? (int)((size_t)B - base) : CH;
    // every wavefront builds the same list from the same ballot: all four leave together or meet at the same barriers
    const bool row = lane < n;
    const bool take = row && (branch[base + (row ? lane : 0)] != 0) != ady;
    const unsigned long long mask = __ballot(take);
    const int total = __popcll(mask);
    if (total == 0) return;
    unsigned short *list = lds.list[wave];
    if (take) list[__popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)lane;
    lds_sync();
    for (int tt = 0; tt * kTileLeaves < total; tt++) {
        const unsigned short *li = list + tt * kTileLeaves;
        const int count = total - tt * kTileLeaves < kTileLeaves ? total - tt * kTileLeaves : kTileLeaves;
        broad_tile(d, weights, t0, t1, lds, count, ady, wave, lane,
                   [&](int lf, int k) { return parent_hidden[(base + li[lf]) * S + k]; },
                   [&](int lf) { return last_action[base + li[lf]]; },
                   [&](int lf) {
                       const size_t r = base + li[lf];
                       return WideDst{hidden_out + r * S, policy_out + r * A, value_out + r, reward_out + r};
                   });
    }
}

template <int CH>
int launch(const smz_mlp_desc *d, const float *weights_dev, const float *parent_hidden_dev, const int32_t *last_action_dev,
           const uint8_t *branch_dev, float *hidden_out_dev, float *reward_out_dev, float *policy_out_dev, float *value_out_dev, int B,
           smz_stream stream) {
    // two activation tiles: 16 KB (H, S <= 128) to 64 KB (H > 384), beside 2.4 KB of static LDS.  HIP caps dynamic LDS at 64 KB
    // unless the kernel opts in; made once per kernel (this instantiation) and size, not per launch (smz_mlp_root.hip)
    const size_t lds = 2 * (size_t)broad_tile_floats(d->S, d->H) * sizeof(float);
    static size_t granted[64] = {};     // per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return SMZ_ERR_HIP;
    if (lds > granted[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp_recurrent_broad<CH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess)
            return SMZ_ERR_HIP;
        granted[dev] = lds;
    }
    hipLaunchKernelGGL(k_mlp_recurrent_broad<CH>, dim3((B + CH - 1) / CH, 2), dim3(kBroadWaves * kWave), lds, (hipStream_t)stream, *d,
                       weights_dev, parent_hidden_dev, last_action_dev, branch_dev, hidden_out_dev, reward_out_dev, policy_out_dev,
                       value_out_dev, B);
    return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
}

}  // namespace

extern "C" {

int smz_mlp_layout_broad(smz_mlp_desc *d) {
    if (!d || d->obs < 1 || d->A < 1 || d->S < 1 || d->H < 1 || d->L < 0) return SMZ_ERR_INVALID;
    if (d->A > SMZ_MAX_ACTIONS_LARGE || d->H > kBroadMaxH || d->S > kBroadMaxS) return SMZ_ERR_TOO_LARGE;
    d->OP = kWideOP;
    const int ph = broad_panels(d->H), ps = broad_panels(d->S), pa = broad_panels(d->A);
    const int rh = broad_r8(d->H), rs = broad_r8(d->S);
    const int mid = d->L > 0 ? ph * rh : 0, pmid = d->L > 0 ? ph : 0;      // one shared Linear(H, H) per trunk, applied L times
    const int in = ph * rs + d->A * ph;                                    // hidden part + one table row of 128 P(H) per action
    // rows of 128 floats per matrix, bias vectors of 128 floats per matrix (= its panels)
    const int rows[M_COUNT] = {in, in, mid, mid, 2 * ps * rh, ps * rh, ph * rs, ph * rs, mid, mid, (pa + ps) * rh, (pa + ps) * rh,
                               ph * broad_r8(d->obs), mid, ps * rh};
    const int vecs[M_COUNT] = {ph, ph, pmid, pmid, 2 * ps, ps, ph, ph, pmid, pmid, pa + ps, pa + ps, ph, pmid, ps};
    int off = 0;
    for (int m = 0; m < M_COUNT; m++) { d->off[m] = off; off += rows[m] * kWideOP; }
    for (int m = 0; m < M_COUNT; m++) { d->off[M_COUNT + m] = off; off += vecs[m] * kWideOP; }
    d->total_floats = off;
    return SMZ_OK;
}

int smz_mlp_recurrent_broad(const smz_mlp_desc *d, const float *weights_dev, const float *parent_hidden_dev,
                            const int32_t *last_action_dev, const uint8_t *branch_dev, float *hidden_out_dev,
                            float *reward_out_dev, float *policy_out_dev, float *value_out_dev, int B, smz_stream stream) {
    if (!d || !weights_dev || !parent_hidden_dev || !last_action_dev || !branch_dev || !hidden_out_dev || !reward_out_dev ||
        !policy_out_dev || !value_out_dev || B < 1)
        return SMZ_ERR_INVALID;
    smz_mlp_desc t = *d;
    if (smz_mlp_layout_broad(&t) != SMZ_OK || t.total_floats != d->total_floats || d->OP != kWideOP) return SMZ_ERR_INVALID;
    for (int m = 0; m < 2 * M_COUNT; m++)
        if (t.off[m] != d->off[m]) return SMZ_ERR_INVALID;
    // chunks of 16 rows up to kBroadSmallMax rows, of 32 above (the header comment; profiles/r16_broad_heads_chunk_ab.txt)
    int small_max = kBroadSmallMax;
    if (const char *e = getenv("SMZ_MLP_BROAD_SMALL_MAX")) small_max = atoi(e);     // (A/B runs: 0 = chunks of 32 rows always)
    return B <= small_max ? launch<kTileLeaves>(d, weights_dev, parent_hidden_dev, last_action_dev, branch_dev, hidden_out_dev,
                                                reward_out_dev, policy_out_dev, value_out_dev, B, stream)
                          : launch<kBroadChunk>(d, weights_dev, parent_hidden_dev, last_action_dev, branch_dev, hidden_out_dev,
                                                reward_out_dev, policy_out_dev, value_out_dev, B, stream);
}

}  // extern "C"
