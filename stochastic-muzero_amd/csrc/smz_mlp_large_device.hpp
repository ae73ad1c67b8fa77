// smz_mlp_large_device.hpp -- device code of the large-action `mlp_model` tile (up to SMZ_MAX_ACTIONS_LARGE actions), shared by
// the stand-alone head kernels (k_mlp_recurrent_large[_split], smz_mlp_large.hip) and the whole-search kernel
// (k_search_mlp_large, smz_mlp_large_search.hip).  Both files are compiled with the same flags (-ffp-contract=off) and a leaf's
// result depends neither on its tile mates nor on its place in the tile, so a leaf goes through the same instructions in the
// same order on either path.  smz_mlp_large.hip's header comment describes the packed image and the panel softmax.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"
#include "smz_mlp_wide_device.hpp"

namespace smz_mlp {

constexpr int kLargeWaves = 4;              // wavefronts per workgroup

__host__ __device__ inline int r8(int k) { return (k + 7) & ~7; }
__host__ __device__ inline int large_panels(int A) { return (A + kWideOP - 1) / kWideOP; }      // policy panels; the value panel follows

// ONE tile of up to 16 leaves of one branch (the large-action counterpart of wide_tile), by one wavefront (PARTS = 1) or by
// the PARTS wavefronts of a workgroup, each with a tile of LDS of its own (part = this wavefront's index; every wavefront of
// the workgroup must call with the same arguments: there are workgroup barriers inside).
//   in(lf, k)   input k < S of leaf lf: the parent's hidden row
//   act(lf)     the leaf's action, as stored (not yet range-checked)
//   dst(lf)     the leaf's destinations; dst.policy doubles as the parking place of the logits
//   xw          PARTS > 1: [PARTS][16][2] floats of LDS where the wavefronts' maxima and sums meet
template <int PARTS, class In, class Act, class Dst>
__device__ inline void large_tile(const smz_mlp_desc &d, const float *__restrict__ weights, float *tile, int count, bool ady, int lane,
                                  int part, float *xw, In in, Act act, Dst dst) {
    const int S = d.S, A = d.A, H = d.H, half = S / 2;
    const int K8h = (H + 7) >> 3, K8s = (S + 7) >> 3;
    // (the lane index taken afresh for every tile: otherwise everything the tails derive from it -- 32 output indices per lane,
    // their support values and comparison masks -- is computed once before the callers' loops and kept in registers across them)
    asm volatile("" : "+v"(lane));
    const int g = lane >> 4, j = lane & 15;
    const bool mine = j < count;
    const WideDst out = dst(mine ? j : 0);
    int a = act(mine ? j : 0);
    if ((unsigned)a >= (unsigned)A) a = 0;                       // never an address: see the header comment
    // the hidden row -> tile, zero beyond it up to the layer's 8-input groups (a ragged tile repeats its first leaf)
    for (int i = lane; i < kTileLeaves * 8 * K8s; i += kWave) {
        const int lf = i / (8 * K8s), k = i % (8 * K8s);
        tile[((k >> 1) * kTileLeaves + lf) * 2 + (k & 1)] = k < S ? in(lf < count ? lf : 0, k) : 0.f;
    }
    lds_sync();
    const WideNets n = wide_nets(d, ady);
    v4f y[kWideTiles];
    wide_layer(weights + n.w_in, weights + n.b_in, tile, K8s, lane, y);
    {   // + row a of the action table behind the hidden part
        const float *row = weights + n.w_in + 8 * K8s * kWideOP + (size_t)a * kWideOP + 4 * g;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++) {
            const float4 w = *reinterpret_cast<const float4 *>(row + 16 * t);
            y[t] = y[t] + v4f{w.x, w.y, w.z, w.w};
        }
    }
    // (the hidden row is stored by part 0 alone; every part holds the same reward)
    const float reward = wide_between(d, weights, n, tile, ady, lane, mine && part == 0, out.hidden, y);
    // policy panels: logits parked in out.policy, running maximum m and sum s of exp(logit - m) over this lane's columns
    const int panels = large_panels(A), panel_floats = 8 * K8h * kWideOP;
    float m = -__builtin_inff(), s = 0.f;
    for (int p = part; p < panels; p += PARTS) {
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
                    if (mine) out.policy[p * kWideOP + o] = y[t][r];
                }
            }
    }
    // the leaf's maximum and sum: over its four lanes, then (PARTS > 1) over the wavefronts in part order
    float mp = tile_max(m);                                      // (-inf: a wavefront without a panel; PARTS = 1: column 0 is finite)
    float dp = wide_sum(m == -__builtin_inff() ? 0.f : s * smz_exp(m - mp));
    if (PARTS > 1) {
        if (g == 0) *reinterpret_cast<float2 *>(xw + (part * kTileLeaves + j) * 2) = make_float2(mp, dp);
        __syncthreads();
        float2 e[PARTS];
#pragma unroll
        for (int q = 0; q < PARTS; q++) e[q] = *reinterpret_cast<const float2 *>(xw + (q * kTileLeaves + j) * 2);
        mp = e[0].x;                                             // (part 0 always has panel 0)
#pragma unroll
        for (int q = 1; q < PARTS; q++) mp = fmaxf(mp, e[q].x);
        dp = 0.f;
#pragma unroll
        for (int q = 0; q < PARTS; q++) dp += e[q].x == -__builtin_inff() ? 0.f : e[q].y * smz_exp(e[q].x - mp);
    }
    if (mine)
        for (int p = part; p < panels; p += PARTS) {
            const int cols = A - p * kWideOP;
#pragma unroll
            for (int t = 0; t < kWideTiles; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int o = 16 * t + 4 * g + r;
                    if (o < cols) {
                        float *q = out.policy + p * kWideOP + o;
                        *q = __fdividef(smz_exp(*q - mp), dp);
                    }
                }
        }
    // the value panel: logits 0..S-1, by the wavefront next in turn
    if (panels % PARTS == part) {                                // (wave-uniform)
        wide_layer(weights + n.wp_out + (size_t)panels * panel_floats, weights + n.bp_out + panels * kWideOP, tile, K8h, lane, y);
        float mv = -__builtin_inff();
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (16 * t + 4 * g + r < S) mv = fmaxf(mv, y[t][r]);
        mv = tile_max(mv);
        float dv = 0.f, nv = 0.f;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 16 * t + 4 * g + r;
                if (o < S) { const float ev = smz_exp(y[t][r] - mv); dv += ev; nv += (float)(o - half) * ev; }
            }
        const float value = support_to_scalar(wide_sum(nv), wide_sum(dv));
        if (mine && g == 0) {
            *out.value = value;
            if (out.reward) *out.reward = reward;
        }
    }
    if (PARTS > 1) __syncthreads();                              // xw is rewritten by the next tile
    lds_sync();
}

}  // namespace smz_mlp
