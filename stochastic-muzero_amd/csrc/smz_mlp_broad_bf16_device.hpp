// smz_mlp_broad_bf16_device.hpp -- device code of the broad `mlp_model` tile with bf16 operands on the matrix cores: broad_tile
// (smz_mlp_broad_device.hpp) with v_mfma_f32_16x16x32_bf16 in the place of v_mfma_f32_16x16x4_f32.  Used by
// k_mlp_recurrent_broad_bf16 (smz_mlp_broad_bf16.hip), whose header comment describes the packed image.
//
// The arithmetic (include/smz.h states it as the contract):
//   * weights and action-table rows are bf16 in the image (rounded to nearest even once, by the host packer); biases are float32;
//   * the input of every Linear layer is rounded to bf16 (v_cvt_pk_bf16_f32, nearest even) where it is written into the LDS
//     activation tile: the parent's hidden row, every ELU(...) output, the scaled next state that feeds the prediction network;
//   * everything else is float32 in the order of broad_tile: the MFMA accumulates in float32 from the bias, one chain per output
//     in input order; the action-table row (a one-hot input times a bf16 weight is that weight) is added to the sums in float32;
//     ELU, minimum / maximum / span, softmax, support decodes, panel-order reductions are broad_tile's statements, and
//     hidden_out receives the UNROUNDED float32 scaled state.
//
// Operand maps of v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15],
// j = 0 .. 7; C/D is col = l & 15, row = 4 (l >> 4) + r.  The weights are the A operand (row = output neuron), the activations the
// B operand (column = leaf): the result is the y[t][r] of wide_layer -- leaf j = lane & 15, neuron 16 t + 4 (lane >> 4) + r -- so
// every reduction and store of broad_tile carries over unchanged.  A lane's fragment is 16 contiguous bytes in both images:
//   * an activation tile is [inputs / 8][16 leaves][8] bf16: lane (g, j) reads the uint4 at (4 s + g) * 16 + j for 32-input step s;
//   * a weight panel is [32-input steps][8 tiles of 16 neurons][64 lanes][8] bf16: one wavefront load of a step's tile is 1 KB of
//     consecutive bytes.
// Inputs are padded to a multiple of 32 with zeros in both images.
//
// As for broad_tile, every wavefront of the workgroup must call broad_bf16_tile with the same arguments: all barriers inside are
// executed by all of them.  A leaf's results depend neither on its tile mates nor on its place in the tile.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"
#include "smz_mlp_wide_device.hpp"
#include "smz_mlp_broad_device.hpp"

namespace smz_mlp {

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

__host__ __device__ inline int bf16_r32(int k) { return (k + 31) & ~31; }
// words (4 bytes) of one panel of a matrix of K inputs: R32(K) x 128 bf16
__host__ __device__ inline int bf16_panel_words(int K) { return bf16_r32(K) * (kWideOP / 2); }
// one activation tile in uint4 (8 bf16): the widest input of any layer, R32(S) or the trunk's 128 P(H), for 16 leaves: at most 16 KB
__host__ __device__ inline int bf16_tile_vecs(int S, int H) {
    const int ks = bf16_r32(S), kh = broad_panels(H) * kWideOP;
    return kTileLeaves * (ks > kh ? ks : kh) / 8;
}

// two floats -> two bf16 (nearest even), the first in the low half
__device__ inline unsigned bf16_pack(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
__device__ inline float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ inline float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// one panel: y = bias + W x over K32 steps of 32 inputs.  W: the panel ([K32][8][64] uint4), xp: the activation tile.
__device__ inline void bf16_layer(const uint4 *__restrict__ W, const float *__restrict__ bias, const uint4 *xp, int K32, int lane,
                                  v4f (&y)[kWideTiles]) {
    const int g = lane >> 4, j = lane & 15;
    uint4 wa[3][kWideTiles];                                // weights of three consecutive steps: two in flight ahead
    const uint4 *Wl = W + lane;
    auto wload = [&](int slot, int s) {
#pragma unroll
        for (int t = 0; t < kWideTiles; t++) wa[slot][t] = Wl[(size_t)(s * kWideTiles + t) * kWave];
    };
#pragma unroll
    for (int t = 0; t < kWideTiles; t++) {
        const float4 b = *reinterpret_cast<const float4 *>(bias + 16 * t + 4 * g);
        y[t] = v4f{b.x, b.y, b.z, b.w};
    }
    wload(0, 0);
    if (K32 > 1) wload(1, 1);
    for (int c = 0; c < K32; c += 3) {                      // three steps per trip: static indices into wa[]
#pragma unroll
        for (int h = 0; h < 3; h++) {
            const int cc = c + h;
            if (cc < K32) {                                 // wave-uniform
                const v8bf xb = __builtin_bit_cast(v8bf, xp[(4 * cc + g) * kTileLeaves + j]);
                if (cc + 2 < K32) wload((h + 2) % 3, cc + 2);
#pragma unroll
                for (int t = 0; t < kWideTiles; t++)
                    y[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, wa[h][t]), xb, y[t], 0, 0, 0);
            }
        }
    }
}

// four consecutive inputs k0 .. k0 + 3 (k0 a multiple of 4) of leaf j, rounded, into the tile
__device__ inline void bf16_tile_store4(uint4 *tile, int k0, int j, float a, float b, float c, float d) {
    reinterpret_cast<uint2 *>(tile)[((k0 >> 3) * kTileLeaves + j) * 2 + ((k0 >> 2) & 1)] = make_uint2(bf16_pack(a, b), bf16_pack(c, d));
}

// ELU of one panel's outputs, rounded, into inputs 128 p .. 128 p + 127 of the tile
__device__ inline void bf16_trunk_store(uint4 *tile, int p, const v4f (&y)[kWideTiles], int lane) {
    const int g = lane >> 4, j = lane & 15;
#pragma unroll
    for (int t = 0; t < kWideTiles; t++)
        bf16_tile_store4(tile, p * kWideOP + 16 * t + 4 * g, j, elu(y[t][0]), elu(y[t][1]), elu(y[t][2]), elu(y[t][3]));
}

// a trunk layer: K32 steps of `src` -> `panels` output panels, ELU, -> `dst`.  Matrix at word W of the image, one bias vector of
// 128 floats per panel at word bias.
__device__ inline void bf16_trunk_layer(const float *__restrict__ image, int W, int bias, const uint4 *src, uint4 *dst, int K32,
                                        int panels, int wave, int lane) {
    v4f y[kWideTiles];
    for (int p = wave; p < panels; p += kBroadWaves) {
        bf16_layer(reinterpret_cast<const uint4 *>(image + W) + (size_t)p * K32 * kWideTiles * kWave, image + bias + p * kWideOP, src,
                   K32, lane, y);
        bf16_trunk_store(dst, p, y, lane);
    }
}

//   image       the packed image as 4-byte words (smz_mlp_layout_broad_bf16): float32 biases, bf16 pairs elsewhere
//   t0, t1      the two activation tiles (bf16_tile_vecs(S, H) uint4 of LDS each)
//   in(lf, k)   input k < S of leaf lf: the parent's hidden row
//   act(lf)     the leaf's action, as stored (not yet range-checked)
//   dst(lf)     the leaf's destinations; dst.policy doubles as the parking place of the logits; dst.reward is never null
template <class In, class Act, class Dst>
__device__ inline void broad_bf16_tile(const smz_mlp_desc &d, const float *__restrict__ image, uint4 *t0, uint4 *t1, BroadLds &lds,
                                       int count, bool ady, int wave, int lane, In in, Act act, Dst dst) {
    const int S = d.S, A = d.A, H = d.H, half = S / 2;
    const int K32h = (H + 31) >> 5, K32s = (S + 31) >> 5;
    const int PH = broad_panels(H), PS = broad_panels(S), PA = broad_panels(A);
    const int panel_h = K32h * kWideTiles * kWave, panel_s = K32s * kWideTiles * kWave;      // uint4 per panel of K = H, K = S
    // (broad_tile's statement, for its reason: without it the per-lane output indices of every stage stay in registers throughout)
    asm volatile("" : "+v"(lane));
    const int g = lane >> 4, j = lane & 15;
    const bool mine = j < count;
    const WideDst out = dst(mine ? j : 0);
    int a = act(mine ? j : 0);
    if ((unsigned)a >= (unsigned)A) a = 0;                       // never an address
    // the hidden rows, rounded, -> tile 0 two inputs at a time, zero beyond them up to the layer's 32-input steps (a ragged tile
    // repeats its first leaf)
    for (int i = wave * kWave + lane; i < kTileLeaves * 16 * K32s; i += kBroadWaves * kWave) {
        const int lf = i / (16 * K32s), k = 2 * (i % (16 * K32s)), lr = lf < count ? lf : 0;
        const float lo = k < S ? in(lr, k) : 0.f, hi = k + 1 < S ? in(lr, k + 1) : 0.f;
        reinterpret_cast<unsigned *>(t0)[((k >> 3) * kTileLeaves + lf) * 4 + ((k & 7) >> 1)] = bf16_pack(lo, hi);
    }
    __syncthreads();
    const WideNets n = wide_nets(d, ady);
    auto mat = [&](int word) { return reinterpret_cast<const uint4 *>(image + word); };
    v4f y[kWideTiles];
    // input layer: the hidden part + row a of the bf16 action table [A][128 PH] behind its PH panels -> tile 1
    for (int p = wave; p < PH; p += kBroadWaves) {
        bf16_layer(mat(n.w_in) + (size_t)p * panel_s, image + n.b_in + p * kWideOP, t0, K32s, lane, y);
        const uint2 *row = reinterpret_cast<const uint2 *>(image + n.w_in + (size_t)PH * panel_s * 4 + ((size_t)a * PH + p) * (kWideOP / 2)) + g;
#pragma unroll
        for (int t = 0; t < kWideTiles; t++) {
            const uint2 w = row[4 * t];
            y[t] = y[t] + v4f{bf16_lo(w.x), bf16_hi(w.x), bf16_lo(w.y), bf16_hi(w.y)};
        }
        bf16_trunk_store(t1, p, y, lane);
    }
    __syncthreads();
    uint4 *src = t1, *oth = t0;
    for (int l = 0; l < d.L; l++) {          // the SAME Linear(H, H) + ELU applied L times
        bf16_trunk_layer(image, n.w_mid, n.b_mid, src, oth, K32h, PH, wave, lane);
        __syncthreads();
        uint4 *x = src; src = oth; oth = x;
    }
    // dynamics output layer: [PS reward panels | PS state panels] (afterstate: PS state panels): at most one per wavefront
    const int PO = ady ? PS : 2 * PS;
    const bool has_out = wave < PO, is_reward = !ady && wave < PS;                     // wave-uniform
    const int ol = is_reward || ady ? wave : wave - PS;                                // the panel's index within its column range
    const int ocols = S - ol * kWideOP;                                                // (> 128: a full panel)
    if (has_out) {
        bf16_layer(mat(n.w_out) + (size_t)wave * panel_h, image + n.b_out + wave * kWideOP, src, K32h, lane, y);
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
        for (int t = 0; t < kWideTiles; t++) {
            const int o0 = 16 * t + 4 * g, k0 = ol * kWideOP + o0;
            if (k0 < 32 * K32s) {                                                      // (inputs S .. 32 K32s - 1: zero)
                float hv[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    hv[r] = o0 + r < ocols ? __fdividef(y[t][r] - mn, sc) : 0.f;
                    if (mine && o0 + r < ocols) out.hidden[k0 + r] = hv[r];            // the float32 state, unrounded
                }
                bf16_tile_store4(oth, k0, j, hv[0], hv[1], hv[2], hv[3]);
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
    { uint4 *x = src; src = oth; oth = x; }
    bf16_trunk_layer(image, n.wp_in, n.bp_in, src, oth, K32s, PH, wave, lane);
    __syncthreads();
    { uint4 *x = src; src = oth; oth = x; }
    for (int l = 0; l < d.L; l++) {
        bf16_trunk_layer(image, n.wp_mid, n.bp_mid, src, oth, K32h, PH, wave, lane);
        __syncthreads();
        uint4 *x = src; src = oth; oth = x;
    }
    // prediction output layer: [PA policy panels | PS value panels]; a wavefront's value panel is its last one
    for (int p = wave; p < PA; p += kBroadWaves) {
        bf16_layer(mat(n.wp_out) + (size_t)p * panel_h, image + n.bp_out + p * kWideOP, src, K32h, lane, y);
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
        bf16_layer(mat(n.wp_out) + (size_t)(PA + vl) * panel_h, image + n.bp_out + (PA + vl) * kWideOP, src, K32h, lane, y);
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
