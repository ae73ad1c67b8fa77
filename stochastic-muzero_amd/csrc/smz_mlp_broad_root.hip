// smz_mlp_broad_root.hip -- the ROOT evaluation of the broad `mlp_model` shapes (H <= 512, S <= 256, A <= 1024) in ONE launch
// (C ABI: smz_mlp_initial_broad): representation, scale_to_bound_action, root prediction trunk, policy softmax -- what
// FusedMlpHeads.initial issues as 12 (L = 0) to 28 (L = 4) library and epilogue launches.  The root value is unused
// (monte_carlo_tree_search.py:319), so the value panels behind the policy panels of pre_out are not read.
//
// The image is that of smz_mlp_layout_broad (smz_mlp_broad.hip), float32: rep_in (K = obs), rep_mid, rep_out, pre_in, pre_mid and
// pre_out are panel matrices, so every layer here is broad_layer's panel scheme (smz_mlp_broad_device.hpp): wavefront w of the
// workgroup takes the output panels w, w + 4, ..., reads the input tile, writes ELU(outputs) into the other tile, and a workgroup
// barrier separates the layers.  What this file adds to the pieces of that header:
//   * the observation tile.  An observation may be wider than any layer of the recurrent networks (up to kBroadRootMaxObs = 1024
//     inputs), so tile 0 is sized for max(R8(obs), 128 P(H), R8(S)) inputs and tile 1 for max(128 P(H), R8(S)): at most
//     64 KB + 32 KB of dynamic LDS, beside 1.3 KB of static LDS.  A workgroup that takes more than half of a CU's 160 KB has
//     the CU to itself; only an observation wider than 744 floats can ask for that.
//   * rep_out (P(S) <= 2 panels, one per wavefront) -> the panels' minima and maxima meet in LDS, every reader combines them in
//     panel order -> span < 1e-5 -> + 1e-5, __fdividef -> hidden_out and the other tile (zeros up to the 8-input group): the
//     statements broad_tile has for its state panels.
//   * the P(A) policy panels of pre_out with the logits parked in policy_out, the panels' maxima and then their sums of
//     exp(x - maximum) combined in panel order: COPIES of the prediction half of broad_tile without its value panels, not a shared
//     function: broad_tile stays as it is, so the kernels of smz_mlp_broad.hip cannot move by an instruction.
// Geometry, the same for every batch size (a row's outputs depend neither on its tile mates, its place in the tile nor on the
// batch): a workgroup of kBroadWaves = 4 wavefronts per 16-row tile, at most kBroadRootMaxWgs workgroups, more tiles
// grid-stride.  The loop is workgroup-uniform: every wavefront meets every barrier, whatever its panel count.
// Compiled with the flags of every unit (-ffp-contract=off).  Outputs are held to the tolerances of the wide kernel against the
// float64 restatement (tests/test_gpu_mlp_broad_root_heads.py), not bit parity with the torch root: the sums run in another order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"
#include "smz_mlp_wide_device.hpp"
#include "smz_mlp_broad_device.hpp"

using namespace smz_mlp;

namespace {

constexpr int kBroadRootMaxObs = 1024;       // widest observation row: a 64 KB tile
constexpr int kBroadRootMaxWgs = 2048;       // grid cap; more tiles than the grid takes in one trip grid-stride

// tile 0 also takes the observations; tile 1 is broad_tile_floats(S, H)
__host__ __device__ inline int broad_root_tile0_floats(int obs, int S, int H) {
    const int a = kTileLeaves * broad_r8(obs), b = broad_tile_floats(S, H);
    return a > b ? a : b;
}

// the static LDS of one workgroup: where the panels' partial results meet
struct BroadRootLds {
    float2 state[kBroadMaxStatePanels][kTileLeaves];            // rep_out panels: (minimum, maximum)
    float pol_max[kBroadMaxPolicyPanels][kTileLeaves], pol_sum[kBroadMaxPolicyPanels][kTileLeaves];
};

// LDS: [tile 0: broad_root_tile0_floats] [tile 1: broad_tile_floats]
__global__ void __launch_bounds__(kBroadWaves *kWave) k_mlp_initial_broad(smz_mlp_desc d, const float *__restrict__ weights,
                                                                          const float *__restrict__ obs, float *__restrict__ hidden_out,
                                                                          float *__restrict__ policy_out, int B) {
    extern __shared__ float4 broad_root_tiles[];
    __shared__ BroadRootLds lds;
    const int OBS = d.obs, S = d.S, A = d.A, H = d.H;
    const int K8o = (OBS + 7) >> 3, K8h = (H + 7) >> 3, K8s = (S + 7) >> 3;
    const int PH = broad_panels(H), PS = broad_panels(S), PA = broad_panels(A);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    float *t0 = reinterpret_cast<float *>(broad_root_tiles), *t1 = t0 + broad_root_tile0_floats(OBS, S, H);
    const int w_in = d.off[M_REP_IN], b_in = d.off[M_COUNT + M_REP_IN], w_mid = d.off[M_REP_MID], b_mid = d.off[M_COUNT + M_REP_MID];
    const int w_out = d.off[M_REP_OUT], b_out = d.off[M_COUNT + M_REP_OUT];
    const int wp_in = d.off[M_PRE_IN], bp_in = d.off[M_COUNT + M_PRE_IN], wp_mid = d.off[M_PRE_MID], bp_mid = d.off[M_COUNT + M_PRE_MID];
    const int wp_out = d.off[M_PRE_OUT], bp_out = d.off[M_COUNT + M_PRE_OUT];
    const int tiles = (B + kTileLeaves - 1) / kTileLeaves;
    for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {         // (workgroup-uniform)
        int lane = threadIdx.x & (kWave - 1);
        asm volatile("" : "+v"(lane));                               // (taken afresh for every tile: see broad_tile)
        const int g = lane >> 4, j = lane & 15;
        const int base = tl * kTileLeaves, count = B - base;         // (may exceed 16: the tile takes the first 16)
        const bool mine = j < count;
        const size_t row = (size_t)base + (mine ? j : 0);
        float *hidden = hidden_out + row * S, *policy = policy_out + row * A;
        // the observations -> tile 0, zero beyond them up to the layer's 8-input groups (a ragged tile repeats its first row)
        for (int i = wave * kWave + lane; i < kTileLeaves * 8 * K8o; i += kBroadWaves * kWave) {
            const int lf = i / (8 * K8o), k = i % (8 * K8o);
            t0[((k >> 1) * kTileLeaves + lf) * 2 + (k & 1)] = k < OBS ? obs[((size_t)base + (lf < count ? lf : 0)) * OBS + k] : 0.f;
        }
        __syncthreads();
        // representation: input layer and trunk
        broad_layer(weights + w_in, weights + b_in, t0, t1, K8o, PH, wave, lane);
        __syncthreads();
        float *src = t1, *oth = t0;
        for (int l = 0; l < d.L; l++) {          // the SAME Linear(H, H) + ELU applied L times
            broad_layer(weights + w_mid, weights + b_mid, src, oth, K8h, PH, wave, lane);
            __syncthreads();
            float *x = src; src = oth; oth = x;
        }
        // representation output layer: PS <= 2 state panels, at most one per wavefront
        v4f y[kWideTiles];
        const bool has_out = wave < PS;                              // wave-uniform
        const int ocols = S - wave * kWideOP;                        // (> 128: a full panel)
        if (has_out) {
            wide_layer(weights + w_out + (size_t)wave * 8 * K8h * kWideOP, weights + b_out + wave * kWideOP, src, K8h, lane, y);
            float mn = __builtin_inff(), mx = -__builtin_inff();
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (16 * t + 4 * g + r < ocols) { mn = fminf(mn, y[t][r]); mx = fmaxf(mx, y[t][r]); }
            mn = tile_min(mn); mx = tile_max(mx);
            if (g == 0) lds.state[wave][j] = make_float2(mn, mx);
        }
        __syncthreads();
        if (has_out) {                           // scale_to_bound_action over all state panels -> the other tile, hidden_out
            float mn = lds.state[0][j].x, mx = lds.state[0][j].y;
            for (int q = 1; q < PS; q++) { mn = fminf(mn, lds.state[q][j].x); mx = fmaxf(mx, lds.state[q][j].y); }
            float sc = mx - mn;
            if (sc < 1e-5f) sc += 1e-5f;
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r, k = wave * kWideOP + o;
                    if (k < 8 * K8s) {                                                     // (inputs S .. 8 K8s - 1: zero)
                        const float hv = o < ocols ? __fdividef(y[t][r] - mn, sc) : 0.f;
                        oth[((k >> 1) * kTileLeaves + j) * 2 + (k & 1)] = hv;
                        if (mine && o < ocols) hidden[k] = hv;
                    }
                }
        }
        __syncthreads();
        // root prediction: input layer and trunk
        { float *x = src; src = oth; oth = x; }
        broad_layer(weights + wp_in, weights + bp_in, src, oth, K8s, PH, wave, lane);
        __syncthreads();
        { float *x = src; src = oth; oth = x; }
        for (int l = 0; l < d.L; l++) {
            broad_layer(weights + wp_mid, weights + bp_mid, src, oth, K8h, PH, wave, lane);
            __syncthreads();
            float *x = src; src = oth; oth = x;
        }
        // the PA policy panels of the prediction output layer: logits parked in `policy`, every panel's maximum to LDS
        const int panel_floats = 8 * K8h * kWideOP;
        for (int p = wave; p < PA; p += kBroadWaves) {
            wide_layer(weights + wp_out + (size_t)p * panel_floats, weights + bp_out + p * kWideOP, src, K8h, lane, y);
            const int cols = A - p * kWideOP;
            float pm = -__builtin_inff();
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r;
                    if (o < cols) {
                        pm = fmaxf(pm, y[t][r]);
                        if (mine) policy[p * kWideOP + o] = y[t][r];
                    }
                }
            pm = tile_max(pm);
            if (g == 0) lds.pol_max[p][j] = pm;
        }
        __syncthreads();
        float mp = lds.pol_max[0][j];            // the row's maximum: over the panels in panel order
        for (int p = 1; p < PA; p++) mp = fmaxf(mp, lds.pol_max[p][j]);
        // every lane re-reads the logits IT wrote (same thread, same addresses: program order)
        for (int p = wave; p < PA; p += kBroadWaves) {
            const int cols = A - p * kWideOP;
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r;
                    if (o < cols) {
                        float *q = policy + p * kWideOP + o;
                        const float e = smz_exp((mine ? *q : mp) - mp);
                        s += e;
                        if (mine) *q = e;
                    }
                }
            s = wide_sum(s);
            if (g == 0) lds.pol_sum[p][j] = s;
        }
        __syncthreads();
        if (mine) {
            float dp = lds.pol_sum[0][j];        // the row's sum: the panels' sums in panel order
            for (int p = 1; p < PA; p++) dp += lds.pol_sum[p][j];
            for (int p = wave; p < PA; p += kBroadWaves) {
                const int cols = A - p * kWideOP;
#pragma unroll
                for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int o = 16 * t + 4 * g + r;
                        if (o < cols) {
                            float *q = policy + p * kWideOP + o;
                            *q = __fdividef(*q, dp);
                        }
                    }
            }
        }
        __syncthreads();                         // the tiles and the meeting places are rewritten by the next trip
    }
}

}  // namespace

extern "C" {

int smz_mlp_initial_broad(const smz_mlp_desc *d, const float *weights_dev, const float *obs_dev, float *hidden_out_dev,
                          float *policy_out_dev, int B, smz_stream stream) {
    // the refusals, before any HIP call
    if (!d || !weights_dev || !obs_dev || !hidden_out_dev || !policy_out_dev || B < 1) return SMZ_ERR_INVALID;
    smz_mlp_desc t = *d;
    if (smz_mlp_layout_broad(&t) != SMZ_OK || t.total_floats != d->total_floats || d->OP != kWideOP) return SMZ_ERR_INVALID;
    for (int m = 0; m < 2 * M_COUNT; m++)
        if (t.off[m] != d->off[m]) return SMZ_ERR_INVALID;
    if (d->obs > kBroadRootMaxObs) return SMZ_ERR_TOO_LARGE;
    // a workgroup per tile: 16 KB (obs, H, S <= 128) to 64 KB + 32 KB (obs 1024, H > 384) of dynamic LDS.  Up to kBroadRootMaxWgs
    // tiles every workgroup makes one trip: row 32 768 starts the second trip of workgroup 0
    // (tests/test_gpu_mlp_broad_root_heads.py runs B = 32 785).  HIP caps dynamic LDS at 64 KB unless the kernel opts in; made
    // once per size, not per launch (smz_mlp_root.hip)
    const size_t lds = ((size_t)broad_root_tile0_floats(d->obs, d->S, d->H) + broad_tile_floats(d->S, d->H)) * sizeof(float);
    static size_t granted[64] = {};     // per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return SMZ_ERR_HIP;
    if (lds > granted[dev]) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_mlp_initial_broad), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess)
            return SMZ_ERR_HIP;
        granted[dev] = lds;
    }
    int wgs = (B + kTileLeaves - 1) / kTileLeaves;
    if (wgs > kBroadRootMaxWgs) wgs = kBroadRootMaxWgs;
    hipLaunchKernelGGL(k_mlp_initial_broad, dim3(wgs), dim3(kBroadWaves * kWave), lds, (hipStream_t)stream, *d, weights_dev, obs_dev,
                       hidden_out_dev, policy_out_dev, B);
    return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
}

}  // extern "C"
