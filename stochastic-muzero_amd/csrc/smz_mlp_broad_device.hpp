// smz_mlp_broad_device.hpp -- device code of the broad `mlp_model` tile (hidden width up to 512, state width up to 256, up to
// SMZ_MAX_ACTIONS_LARGE actions): EVERY layer is a sequence of 128-column output panels, each a matrix wide_layer
// (smz_mlp_wide_device.hpp) takes as it is, and the reductions that sit between the layers -- the minimum and maximum of
// scale_to_bound_action, the reward and value support decodes, the policy softmax -- run across panels.  Used by
// k_mlp_recurrent_broad (smz_mlp_broad.hip), whose header comment describes the packed image.
//
// One tile = up to 16 leaves of one branch, by the kBroadWaves wavefronts of a workgroup together:
//   * two activation tiles in LDS in ping-pong, [inputs / 2][16 leaves][2] floats each (the input layout of wide_layer), shared
//     by the whole workgroup.  For every layer wavefront w takes the output panels p = w, w + 4, ...: it reads the input tile,
//     holds the panel's 64 accumulators and writes ELU(outputs) into inputs 128 p .. 128 p + 127 of the OTHER tile; a workgroup
//     barrier separates the layers.  Output columns beyond the layer's width have zero weights and a zero bias, so they store
//     ELU(0) = 0: the padding inputs of the next layer.
//   * a reduction across panels goes through LDS in two steps: every panel's wavefront reduces its own columns (tile_max /
//     tile_min / wide_sum over the four lanes of a leaf) and stores the panel's partial result; after a barrier every reader
//     combines the partial results IN PANEL ORDER -- maxima first, then sums of exp(x - maximum) -- so the bits do not depend on
//     which wavefront computed which panel.
//   * the dynamics output layer has at most four panels (reward logits: ceil(S / 128) <= 2, next state: as many) and the value
//     logits at most two, which come last in their wavefronts' panel sequences: a wavefront holds such a panel's sums in
//     registers across the barriers of its reduction.  Policy logits are parked in policy_out (as the large-action kernel does):
//     every lane re-reads only what it wrote itself.
// Every wavefront of the workgroup must call broad_tile with the same arguments: all barriers inside are executed by all of
// them, whatever their panel count.  A leaf's results depend neither on its tile mates nor on its place in the tile.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"
#include "smz_mlp_wide_device.hpp"

namespace smz_mlp {

constexpr int kBroadWaves = 4;                        // wavefronts per workgroup
constexpr int kBroadMaxH = 512, kBroadMaxS = 256;     // the envelope of smz_mlp_layout_broad
// one activation tile: the widest input of any layer, R8(S) or the trunk's 128 P(H) (which covers R8(H)), for 16 leaves: at
// most 32 KB.  The two tiles are the workgroup's dynamic LDS.
__host__ __device__ inline int broad_tile_floats(int S, int H) {
    const int ks = (S + 7) & ~7, kh = (H + kWideOP - 1) / kWideOP * kWideOP;
    return kTileLeaves * (ks > kh ? ks : kh);
}
constexpr int kBroadMaxPolicyPanels = SMZ_MAX_ACTIONS_LARGE / kWideOP;
constexpr int kBroadMaxStatePanels = kBroadMaxS / kWideOP;

__host__ __device__ inline int broad_r8(int k) { return (k + 7) & ~7; }
__host__ __device__ inline int broad_panels(int n) { return (n + kWideOP - 1) / kWideOP; }

// the static LDS of one workgroup: where the panels' partial results meet, and the row lists
struct BroadLds {
    float2 out_a[2 * kBroadMaxStatePanels][kTileLeaves];        // dynamics output panels: (maximum, -) reward, (minimum, maximum) state
    float2 out_b[kBroadMaxStatePanels][kTileLeaves];            // reward panels: (numerator, denominator)
    float pol_max[kBroadMaxPolicyPanels][kTileLeaves], pol_sum[kBroadMaxPolicyPanels][kTileLeaves];
    float val_max[kBroadMaxStatePanels][kTileLeaves];
    float2 val_sum[kBroadMaxStatePanels][kTileLeaves];          // value panels: (numerator, denominator)
    unsigned short list[kBroadWaves][2 * kTileLeaves];          // a list of the chunk's rows per wavefront (all four alike)
};

// ELU of one panel's outputs into inputs 128 p .. 128 p + 127 of the tile
__device__ inline void broad_trunk_store(float *tile, int p, const v4f (&y)[kWideTiles], int lane) {
    wide_trunk_store(tile + p * (kWideOP / 2) * kTileLeaves * 2, y, lane);
}

// a trunk layer: K8 eight-input groups of `src` -> `panels` output panels, ELU, -> `dst`.  Matrix at W (a panel after the
// other, 8 K8 x 128 floats each), one bias vector of 128 floats per panel at bias.
__device__ inline void broad_layer(const float *__restrict__ W, const float *__restrict__ bias, const float *src, float *dst, int K8,
                                   int panels, int wave, int lane) {
    v4f y[kWideTiles];
    for (int p = wave; p < panels; p += kBroadWaves) {
        wide_layer(W + (size_t)p * 8 * K8 * kWideOP, bias + p * kWideOP, src, K8, lane, y);
        broad_trunk_store(dst, p, y, lane);
    }
}

//   t0, t1      the two activation tiles (broad_tile_floats(S, H) floats of LDS each)
//   in(lf, k)   input k < S of leaf lf: the parent's hidden row
//   act(lf)     the leaf's action, as stored (not yet range-checked)
//   dst(lf)     the leaf's destinations; dst.policy doubles as the parking place of the logits; dst.reward is never null
template <class In, class Act, class Dst>
__device__ inline void broad_tile(const smz_mlp_desc &d, const float *__restrict__ weights, float *t0, float *t1, BroadLds &lds,
                                  int count, bool ady, int wave, int lane, In in, Act act, Dst dst) {
    const int S = d.S, A = d.A, H = d.H, half = S / 2;
    const int K8h = (H + 7) >> 3, K8s = (S + 7) >> 3;
    const int PH = broad_panels(H), PS = broad_panels(S), PA = broad_panels(A);
    // (large_tile's statement, for its reason: otherwise everything the stages derive from the lane index -- 32 output indices per
    // lane, their support values and comparison masks, for every stage -- is computed once and kept in registers throughout:
    // about 415 vector registers instead of about 210, one wavefront per SIMD instead of two)
    asm volatile("" : "+v"(lane));
    const int g = lane >> 4, j = lane & 15;
    const bool mine = j < count;
    const WideDst out = dst(mine ? j : 0);
    int a = act(mine ? j : 0);
    if ((unsigned)a >= (unsigned)A) a = 0;                       // never an address
    // the hidden rows -> tile 0, zero beyond them up to the layer's 8-input groups (a ragged tile repeats its first leaf)
    for (int i = wave * kWave + lane; i < kTileLeaves * 8 * K8s; i += kBroadWaves * kWave) {
        const int lf = i / (8 * K8s), k = i % (8 * K8s);
        t0[((k >> 1) * kTileLeaves + lf) * 2 + (k & 1)] = k < S ? in(lf < count ? lf : 0, k) : 0.f;
    }
    __syncthreads();
    const WideNets n = wide_nets(d, ady);
    v4f y[kWideTiles];
    // input layer: the hidden part + row a of the action table [A][128 PH] behind its PH panels -> tile 1
    for (int p = wave; p < PH; p += kBroadWaves) {
        wide_layer(weights + n.w_in + (size_t)p * 8 * K8s * kWideOP, weights + n.b_in + p * kWideOP, t0, K8s, lane, y);
        const float *row = weights + n.w_in + (size_t)PH * 8 * K8s * kWideOP + (size_t)a * PH * kWideOP + p * kWideOP + 4 * g;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++) {
            const float4 w = *reinterpret_cast<const float4 *>(row + 16 * t);
            y[t] = y[t] + v4f{w.x, w.y, w.z, w.w};
        }
        broad_trunk_store(t1, p, y, lane);
    }
    __syncthreads();
    float *src = t1, *oth = t0;
    for (int l = 0; l < d.L; l++) {          // the SAME Linear(H, H) + ELU applied L times
        broad_layer(weights + n.w_mid, weights + n.b_mid, src, oth, K8h, PH, wave, lane);
        __syncthreads();
        float *x = src; src = oth; oth = x;
    }
    // dynamics output layer: [PS reward panels | PS state panels] (afterstate: PS state panels): at most one per wavefront
    const int PO = ady ? PS : 2 * PS;
    const bool has_out = wave < PO, is_reward = !ady && wave < PS;                     // wave-uniform
    const int ol = is_reward || ady ? wave : wave - PS;                                // the panel's index within its column range
    const int ocols = S - ol * kWideOP;                                                // (> 128: a full panel)
    if (has_out) {
        wide_layer(weights + n.w_out + (size_t)wave * 8 * K8h * kWideOP, weights + n.b_out + wave * kWideOP, src, K8h, lane, y);
        float mn = __builtin_inff(), mx = -__builtin_inff();
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (16 * t + 4 * g + r < ocols) { mn = fminf(mn, y[t][r]); mx = fmaxf(mx, y[t][r]); }
        mn = tile_min(mn); mx = tile_max(mx);
        if (g == 0) lds.out_a[wave][j] = is_reward ? make_float2(mx, 0.f) : make_float2(mn, mx);
    }
    __syncthreads();
    if (is_reward) {
        float mr = lds.out_a[0][j].x;
        for (int q = 1; q < PS; q++) mr = fmaxf(mr, lds.out_a[q][j].x);
        float den = 0.f, num = 0.f;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r;
                if (o < ocols) { const float ev = smz_exp(y[t][r] - mr); den += ev; num += (float)(ol * kWideOP + o - half) * ev; }
            }
        num = wide_sum(num); den = wide_sum(den);
        if (g == 0) lds.out_b[wave][j] = make_float2(num, den);
    } else if (has_out) {                    // a state panel: scale_to_bound_action over all state panels -> the other tile, hidden_out
        const int q0 = ady ? 0 : PS;
        float mn = lds.out_a[q0][j].x, mx = lds.out_a[q0][j].y;
        for (int q = 1; q < PS; q++) { mn = fminf(mn, lds.out_a[q0 + q][j].x); mx = fmaxf(mx, lds.out_a[q0 + q][j].y); }
        float sc = mx - mn;
        if (sc < 1e-5f) sc += 1e-5f;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r, k = ol * kWideOP + o;
                if (k < 8 * K8s) {                                                     // (inputs S .. 8 K8s - 1: zero)
                    const float hv = o < ocols ? __fdividef(y[t][r] - mn, sc) : 0.f;
                    oth[((k >> 1) * kTileLeaves + j) * 2 + (k & 1)] = hv;
                    if (mine && o < ocols) out.hidden[k] = hv;
                }
            }
    }
    __syncthreads();
    if (wave == 0 && g == 0 && mine) {       // the reward: the panels' sums in panel order (0 on the afterstate branch)
        float reward = 0.f;
        if (!ady) {
            float num = lds.out_b[0][j].x, den = lds.out_b[0][j].y;
            for (int q = 1; q < PS; q++) { num += lds.out_b[q][j].x; den += lds.out_b[q][j].y; }
            reward = support_to_scalar(num, den);
        }
        *out.reward = reward;
    }
    // prediction input layer and trunk
    { float *x = src; src = oth; oth = x; }
    broad_layer(weights + n.wp_in, weights + n.bp_in, src, oth, K8s, PH, wave, lane);
    __syncthreads();
    { float *x = src; src = oth; oth = x; }
    for (int l = 0; l < d.L; l++) {
        broad_layer(weights + n.wp_mid, weights + n.bp_mid, src, oth, K8h, PH, wave, lane);
        __syncthreads();
        float *x = src; src = oth; oth = x;
    }
    // prediction output layer: [PA policy panels | PS value panels]; a wavefront's value panel is its last one
    const int panel_floats = 8 * K8h * kWideOP;
    for (int p = wave; p < PA; p += kBroadWaves) {
        wide_layer(weights + n.wp_out + (size_t)p * panel_floats, weights + n.bp_out + p * kWideOP, src, K8h, lane, y);
        const int cols = A - p * kWideOP;
        float pm = -__builtin_inff();
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r;
                if (o < cols) {
                    pm = fmaxf(pm, y[t][r]);
                    if (mine) out.policy[p * kWideOP + o] = y[t][r];
                }
            }
        pm = tile_max(pm);
        if (g == 0) lds.pol_max[p][j] = pm;
    }
    const int vl = (wave - PA % kBroadWaves + kBroadWaves) % kBroadWaves;              // this wavefront's value panel, if < PS
    const bool has_val = vl < PS;                                                      // wave-uniform
    const int vcols = S - vl * kWideOP;
    if (has_val) {
        wide_layer(weights + n.wp_out + (size_t)(PA + vl) * panel_floats, weights + n.bp_out + (PA + vl) * kWideOP, src, K8h, lane, y);
        float mv = -__builtin_inff();
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (16 * t + 4 * g + r < vcols) mv = fmaxf(mv, y[t][r]);
        mv = tile_max(mv);
        if (g == 0) lds.val_max[vl][j] = mv;
    }
    __syncthreads();
    float mp = lds.pol_max[0][j];            // the leaf's maximum: over the panels in panel order
    for (int p = 1; p < PA; p++) mp = fmaxf(mp, lds.pol_max[p][j]);
    for (int p = wave; p < PA; p += kBroadWaves) {
        const int cols = A - p * kWideOP;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r;
                if (o < cols) {
                    float *q = out.policy + p * kWideOP + o;
                    const float e = smz_exp((mine ? *q : mp) - mp);
                    s += e;
                    if (mine) *q = e;
                }
            }
        s = wide_sum(s);
        if (g == 0) lds.pol_sum[p][j] = s;
    }
    if (has_val) {
        float mv = lds.val_max[0][j];
        for (int q = 1; q < PS; q++) mv = fmaxf(mv, lds.val_max[q][j]);
        float dv = 0.f, nv = 0.f;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r;
                if (o < vcols) { const float ev = smz_exp(y[t][r] - mv); dv += ev; nv += (float)(vl * kWideOP + o - half) * ev; }
            }
        nv = wide_sum(nv); dv = wide_sum(dv);
        if (g == 0) lds.val_sum[vl][j] = make_float2(nv, dv);
    }
    __syncthreads();
    if (mine) {
        float dp = lds.pol_sum[0][j];        // the leaf's sum: the panels' sums in panel order
        for (int p = 1; p < PA; p++) dp += lds.pol_sum[p][j];
        for (int p = wave; p < PA; p += kBroadWaves) {
            const int cols = A - p * kWideOP;
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r;
                    if (o < cols) {
                        float *q = out.policy + p * kWideOP + o;
                        *q = __fdividef(*q, dp);
                    }
                }
        }
        if (has_val && vl == 0 && g == 0) {
            float nv = lds.val_sum[0][j].x, dv = lds.val_sum[0][j].y;
            for (int q = 1; q < PS; q++) { nv += lds.val_sum[q][j].x; dv += lds.val_sum[q][j].y; }
            *out.value = support_to_scalar(nv, dv);
        }
    }
    __syncthreads();                         // the tiles and the meeting places are rewritten by the next tile
}

}  // namespace smz_mlp
