// smz_mlp_root.hip -- the ROOT evaluation of the wide and the large-action `mlp_model` shapes in ONE launch
// (C ABI: smz_mlp_initial_wide / smz_mlp_initial_large): representation, scale_to_bound_action, root prediction trunk, policy
// softmax -- what FusedMlpHeads.initial issues as 12 (L = 0) to 28 (L = 4) library and epilogue launches.  The root value is
// unused (monte_carlo_tree_search.py:319), so the value columns / the value panel are not computed.
//
// Both packed images (smz_mlp_layout_wide, smz_mlp_layout_large) carry rep_in, rep_mid and rep_out as plain wide matrices, and
// wide_between (smz_mlp_wide_device.hpp) is "trunk -> output layer -> scale_to_bound_action -> store hidden row -> next network's
// input layer and trunk".  Given a WideNets whose first half names the representation matrices and whose second half names the
// root prediction's, and the afterstate column placement (state in columns 0..S-1, no reward), it is the root evaluation up to
// the policy layer.  This file adds what stands in front of it and behind it:
//   * the observation input layer: wide_layer over rep_in with K8 = R8(obs) / 8 on an observation tile of 16 R8(obs) floats in
//     wide_layer's input order.  An observation may be wider than the 128 inputs of the 8 KB tile of the other kernels (361 for
//     a Go board, up to kRootMaxObs = 1024: a 64 KB tile); LDS is sized by the launcher.
//   * wide policy: one wide_layer over pre_out [policy | value], softmax over the columns < A (the tail of wide_tile without its
//     value half).
//   * large policy: the ceil(A / 128) policy panels with the running-maximum / running-sum softmax, logits parked in policy_out.
//     These are COPIES of the panel statements of large_tile (smz_mlp_large_device.hpp), not a shared function: large_tile stays as it
//     is, so the two k_mlp_recurrent_large* kernels cannot move by an instruction, and the copy drops what the root does not
//     need (the action table, the value panel, the choice of PARTS).
// Geometry, one per layout, the same for every batch size (a row's outputs depend neither on its tile mates nor on the batch):
//   * k_mlp_initial_wide: a wavefront per 16-row tile on a tile of max(kWideTileFloats, 16 R8(obs)) floats of its own -- after
//     the input layer its first kWideTileFloats serve the 128-wide layers -- four wavefronts per workgroup while four such tiles
//     fit the 160 KB of a CU (obs <= 640), two above; every wavefront strides over the tiles by itself (no workgroup barrier).
//   * k_mlp_initial_large: a workgroup of four wavefronts per tile (what k_mlp_recurrent_large_split does for the recurrent
//     networks).  The workgroup stages ONE observation tile, every wavefront computes the trunk for itself on a private 8 KB
//     tile (the same bits four times: cheaper than passing it round) and takes every fourth panel; maxima and sums meet in LDS
//     in a fixed order.  Measured against one wavefront per tile (profiles/r14_root_heads_split_ab.txt): 47 instead of 82 us at
//     (361,362,32,64,1) and 44 instead of 120 us at (4,1024,16,64,1), at 256 to 4096 rows -- a panel's softmax is 32
//     exponentials per lane around two passes of scattered 4-byte accesses to policy_out.
// Compiled with the flags of every unit (-ffp-contract=off).  Outputs are held to the tolerances of the wide kernel against the
// float64 restatement (tests/test_gpu_mlp_root_heads.py), not bit parity with the torch root: the sums run in another order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"
#include "smz_mlp_wide_device.hpp"
#include "smz_mlp_large_device.hpp"          // r8

using namespace smz_mlp;

namespace {

constexpr int kRootWaves = 4;                // wavefronts per workgroup (one per SIMD)
constexpr int kRootMaxObs = 1024;            // widest observation row: a 64 KB tile
constexpr int kRootMaxWgs = 2048;            // grid cap; more tiles than the grid takes in one trip grid-stride
constexpr int kRootLdsBytes = 160 * 1024;

__host__ __device__ inline int root_tile_floats(int obs) {
    const int f = kTileLeaves * r8(obs);
    return f > kWideTileFloats ? f : kWideTileFloats;
}

// representation -> slots of the (afterstate) dynamics, root prediction -> slots of the prediction
__device__ inline WideNets root_nets(const smz_mlp_desc &d) {
    WideNets n;
    n.w_in = d.off[M_REP_IN]; n.b_in = d.off[M_COUNT + M_REP_IN];
    n.w_mid = d.off[M_REP_MID]; n.b_mid = d.off[M_COUNT + M_REP_MID];
    n.w_out = d.off[M_REP_OUT]; n.b_out = d.off[M_COUNT + M_REP_OUT];
    n.wp_in = d.off[M_PRE_IN]; n.bp_in = d.off[M_COUNT + M_PRE_IN];
    n.wp_mid = d.off[M_PRE_MID]; n.bp_mid = d.off[M_COUNT + M_PRE_MID];
    n.wp_out = d.off[M_PRE_OUT]; n.bp_out = d.off[M_COUNT + M_PRE_OUT];
    return n;
}

// observations of the tile's rows -> `tile` in wide_layer's input order [k/2][16 rows][2], zero beyond them up to the layer's
// 8-input groups, by `threads` threads of which this is `thread`.  A ragged tile (count < 16) repeats its first row.
__device__ inline void root_stage(float *tile, const float *__restrict__ obs, int OBS, int base, int count, int thread, int threads) {
    const int K = (OBS + 7) & ~7;
    for (int i = thread; i < kTileLeaves * K; i += threads) {
        const int lf = i / K, k = i % K;
        tile[((k >> 1) * kTileLeaves + lf) * 2 + (k & 1)] = k < OBS ? obs[((size_t)base + (lf < count ? lf : 0)) * OBS + k] : 0.f;
    }
}

// an image of smz_mlp_layout_wide; LDS: [waves][tile_floats]
__global__ void __launch_bounds__(kRootWaves *kWave) k_mlp_initial_wide(smz_mlp_desc d, const float *__restrict__ weights,
                                                                        const float *__restrict__ obs, float *__restrict__ hidden_out,
                                                                        float *__restrict__ policy_out, int B, int tile_floats) {
    extern __shared__ float4 smz_root_lds4[];
    const int OBS = d.obs, S = d.S, A = d.A, H = d.H;
    const int K8o = (OBS + 7) >> 3, K8h = (H + 7) >> 3;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), waves = blockDim.x / kWave;
    float *tile = reinterpret_cast<float *>(smz_root_lds4) + (size_t)wave * tile_floats;
    const WideNets n = root_nets(d);
    const int tiles = (B + kTileLeaves - 1) / kTileLeaves;
    for (int tl = blockIdx.x * waves + wave; tl < tiles; tl += gridDim.x * waves) {      // (wave-uniform)
        int lane = threadIdx.x & (kWave - 1);
        asm volatile("" : "+v"(lane));                               // (taken afresh for every tile: see large_tile)
        const int g = lane >> 4, j = lane & 15;
        const int base = tl * kTileLeaves, count = B - base;         // (may exceed 16: the tile takes the first 16)
        const bool mine = j < count;
        const size_t row = (size_t)base + (mine ? j : 0);
        root_stage(tile, obs, OBS, base, count, lane, kWave);
        lds_sync();
        v4f y[kWideTiles];
        wide_layer(weights + n.w_in, weights + n.b_in, tile, K8o, lane, y);
        wide_between(d, weights, n, tile, true, lane, mine, hidden_out + row * S, y);
        wide_layer(weights + n.wp_out, weights + n.bp_out, tile, K8h, lane, y);
        float mp = -__builtin_inff();
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (16 * t + 4 * g + r < A) mp = fmaxf(mp, y[t][r]);
        mp = tile_max(mp);
        float dp = 0.f;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (16 * t + 4 * g + r < A) { y[t][r] = smz_exp(y[t][r] - mp); dp += y[t][r]; }
        dp = wide_sum(dp);
        if (mine) {
            float *policy = policy_out + row * A;
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r;
                    if (o < A) policy[o] = __fdividef(y[t][r], dp);
                }
        }
        lds_sync();                                                  // the tile is restaged for the next trip
    }
}

// an image of smz_mlp_layout_large; one workgroup of kRootWaves wavefronts per tile, the loop is workgroup-uniform: every
// wavefront meets every barrier.  LDS: [observation tile: 16 R8(obs)] [kRootWaves][kWideTileFloats] [kRootWaves][16] (max, sum)
__global__ void __launch_bounds__(kRootWaves *kWave) k_mlp_initial_large(smz_mlp_desc d, const float *__restrict__ weights,
                                                                         const float *__restrict__ obs, float *__restrict__ hidden_out,
                                                                         float *__restrict__ policy_out, int B) {
    extern __shared__ float4 smz_root_lds4[];
    const int OBS = d.obs, S = d.S, A = d.A, H = d.H;
    const int K8o = (OBS + 7) >> 3, K8h = (H + 7) >> 3;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    float *otile = reinterpret_cast<float *>(smz_root_lds4);
    float *tile = otile + kTileLeaves * 8 * K8o + part * kWideTileFloats;
    float *xw = otile + kTileLeaves * 8 * K8o + kRootWaves * kWideTileFloats;
    const WideNets n = root_nets(d);
    const int tiles = (B + kTileLeaves - 1) / kTileLeaves;
    for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {         // (workgroup-uniform)
        int lane = threadIdx.x & (kWave - 1);
        asm volatile("" : "+v"(lane));                               // (taken afresh for every tile: see large_tile)
        const int g = lane >> 4, j = lane & 15;
        const int base = tl * kTileLeaves, count = B - base;
        const bool mine = j < count;
        const size_t row = (size_t)base + (mine ? j : 0);
        root_stage(otile, obs, OBS, base, count, threadIdx.x, kRootWaves * kWave);
        __syncthreads();
        v4f y[kWideTiles];
        wide_layer(weights + n.w_in, weights + n.b_in, otile, K8o, lane, y);
        // (the hidden row is stored by part 0 alone; every part holds the same trunk in its own tile)
        wide_between(d, weights, n, tile, true, lane, mine && part == 0, hidden_out + row * S, y);
        // policy panels: logits parked in `policy`, running maximum m and sum s of exp(logit - m) over this lane's columns
        float *policy = policy_out + row * A;
        const int panels = (A + kWideOP - 1) / kWideOP, panel_floats = 8 * K8h * kWideOP;
        float m = -__builtin_inff(), s = 0.f;
        for (int p = part; p < panels; p += kRootWaves) {
            wide_layer(weights + n.wp_out + (size_t)p * panel_floats, weights + n.bp_out + p * kWideOP, tile, K8h, lane, y);
            const int cols = A - p * kWideOP;                        // (> 128: a full panel)
            float pm = m;
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (16 * t + 4 * g + r < cols) pm = fmaxf(pm, y[t][r]);
            s = m == -__builtin_inff() ? 0.f : s * smz_exp(m - pm);
            m = pm;
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r;
                    if (o < cols) {
                        s += smz_exp(y[t][r] - m);
                        if (mine) policy[p * kWideOP + o] = y[t][r];
                    }
                }
        }
        // the row's maximum and sum: over its four lanes, then over the wavefronts in part order (-inf: a wavefront without a panel)
        float mp = tile_max(m);
        float dp = wide_sum(m == -__builtin_inff() ? 0.f : s * smz_exp(m - mp));
        if (g == 0) *reinterpret_cast<float2 *>(xw + (part * kTileLeaves + j) * 2) = make_float2(mp, dp);
        __syncthreads();
        float2 e[kRootWaves];
#pragma unroll
        for (int q = 0; q < kRootWaves; q++) e[q] = *reinterpret_cast<const float2 *>(xw + (q * kTileLeaves + j) * 2);
        mp = e[0].x;                                                 // (part 0 always has panel 0)
#pragma unroll
        for (int q = 1; q < kRootWaves; q++) mp = fmaxf(mp, e[q].x);
        dp = 0.f;
#pragma unroll
        for (int q = 0; q < kRootWaves; q++) dp += e[q].x == -__builtin_inff() ? 0.f : e[q].y * smz_exp(e[q].x - mp);
        // every lane re-reads the logits IT wrote (same thread, same addresses: program order)
        if (mine)
            for (int p = part; p < panels; p += kRootWaves) {
                const int cols = A - p * kWideOP;
#pragma unroll
                for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int o = 16 * t + 4 * g + r;
                        if (o < cols) {
                            float *q = policy + p * kWideOP + o;
                            *q = __fdividef(smz_exp(*q - mp), dp);
                        }
                    }
            }
        __syncthreads();                                             // the observation tile and xw are rewritten by the next trip
    }
}

template <typename Kern>
int allow_lds(Kern kern, size_t bytes) {
    // HIP caps dynamic LDS at 64 KB unless the kernel opts in; made once per kernel and size, not per launch (smz_mlp.hip)
    static size_t granted[64] = {};     // per device
    static const void *who[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return SMZ_ERR_HIP;
    if (who[dev] == reinterpret_cast<const void *>(kern) && bytes <= granted[dev]) return SMZ_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
        hipSuccess)
        return SMZ_ERR_HIP;
    who[dev] = reinterpret_cast<const void *>(kern);
    granted[dev] = bytes;
    return SMZ_OK;
}

// the refusals both entry points make before any HIP call
int root_check(bool large, const smz_mlp_desc *d, const float *weights_dev, const float *obs_dev, float *hidden_out_dev,
               float *policy_out_dev, int B) {
    if (!d || !weights_dev || !obs_dev || !hidden_out_dev || !policy_out_dev || B < 1) return SMZ_ERR_INVALID;
    smz_mlp_desc t = *d;
    if ((large ? smz_mlp_layout_large(&t) : smz_mlp_layout_wide(&t)) != SMZ_OK || t.total_floats != d->total_floats ||
        d->OP != kWideOP)
        return SMZ_ERR_INVALID;
    for (int m = 0; m < 2 * M_COUNT; m++)
        if (t.off[m] != d->off[m]) return SMZ_ERR_INVALID;
    return d->obs > kRootMaxObs ? SMZ_ERR_TOO_LARGE : SMZ_OK;
}

}  // namespace

extern "C" {

int smz_mlp_initial_wide(const smz_mlp_desc *d, const float *weights_dev, const float *obs_dev, float *hidden_out_dev,
                         float *policy_out_dev, int B, smz_stream stream) {
    if (const int rc = root_check(false, d, weights_dev, obs_dev, hidden_out_dev, policy_out_dev, B)) return rc;
    // four wavefronts per workgroup while four observation tiles fit the 160 KB of a CU (obs <= 640), two above (obs 1024:
    // 2 x 64 KB).  Up to kRootMaxWgs * waves tiles every wavefront makes one trip: with four wavefronts row 131 072 starts the
    // second trip of workgroup 0's first wavefront (tests/test_gpu_mlp_root_heads.py runs B = 131 089).
    const int tile_floats = root_tile_floats(d->obs);
    const int waves = (size_t)kRootWaves * tile_floats * sizeof(float) <= (size_t)kRootLdsBytes ? kRootWaves : 2;
    const size_t lds = (size_t)waves * tile_floats * sizeof(float);
    const int tiles = (B + kTileLeaves - 1) / kTileLeaves;
    int wgs = (tiles + waves - 1) / waves;
    if (wgs > kRootMaxWgs) wgs = kRootMaxWgs;
    if (allow_lds(k_mlp_initial_wide, lds) != SMZ_OK) return SMZ_ERR_HIP;
    hipLaunchKernelGGL(k_mlp_initial_wide, dim3(wgs), dim3(waves * kWave), lds, (hipStream_t)stream, *d, weights_dev, obs_dev,
                       hidden_out_dev, policy_out_dev, B, tile_floats);
    return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
}

int smz_mlp_initial_large(const smz_mlp_desc *d, const float *weights_dev, const float *obs_dev, float *hidden_out_dev,
                          float *policy_out_dev, int B, smz_stream stream) {
    if (const int rc = root_check(true, d, weights_dev, obs_dev, hidden_out_dev, policy_out_dev, B)) return rc;
    // a workgroup per tile: at most 64 KB + 32 KB + 512 bytes of LDS (obs 1024).  Up to kRootMaxWgs tiles every workgroup makes
    // one trip: row 32 768 starts the second trip of workgroup 0 (tests/test_gpu_mlp_root_heads.py runs B = 32 785).
    const size_t lds = ((size_t)kTileLeaves * r8(d->obs) + kRootWaves * kWideTileFloats + kRootWaves * kTileLeaves * 2) * sizeof(float);
    int wgs = (B + kTileLeaves - 1) / kTileLeaves;
    if (wgs > kRootMaxWgs) wgs = kRootMaxWgs;
    if (allow_lds(k_mlp_initial_large, lds) != SMZ_OK) return SMZ_ERR_HIP;
    hipLaunchKernelGGL(k_mlp_initial_large, dim3(wgs), dim3(kRootWaves * kWave), lds, (hipStream_t)stream, *d, weights_dev, obs_dev,
                       hidden_out_dev, policy_out_dev, B);
    return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
}

}  // extern "C"
