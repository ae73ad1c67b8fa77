// smz_mlp_broad_bf16.hip -- the broad recurrent `mlp_model` networks (smz_mlp_broad.hip: 1 <= H <= 512, 1 <= S <= 256,
// 1 <= A <= SMZ_MAX_ACTIONS_LARGE, one launch per simulation round) with bf16 operands on the matrix cores
// (C ABI: smz_mlp_layout_broad_bf16 / smz_mlp_recurrent_broad_bf16).  v_mfma_f32_16x16x32_bf16 issues at 16 times the rate of the
// float32-input MFMA of the float32 kernel, and a tile streams half the weight bytes from L2.
//
// The arithmetic is a contract of its own (include/smz.h; smz_mlp_broad_bf16_device.hpp): bf16 weights, every Linear input rounded
// to bf16 where it enters the LDS tile, float32 for everything else.  It is not torch.autocast's.
//
// The packed image (smz_mlp_layout_broad_bf16), in 4-byte words: biases are float32 words, everything else pairs of bf16 (element
// e of a piece at word base: bits 16 (e % 2) .. 16 (e % 2) + 15 of word base + e / 2).  R32(x) = x rounded up to a multiple of
// 32, P(n) = ceil(n / 128).  A "panel matrix" of K inputs and O outputs at base, with its biases at bias, is P(O) panels of
// R32(K) x 128 bf16 (R32(K) * 64 words) each; panel p holds output columns 128 p .. min(O, 128 p + 128) - 1 as R32(K) / 32 steps
// of 32 inputs, a step as 8 tiles of 16 outputs, a tile as the 64 operand fragments of 8 bf16 of the MFMA:
//     weight (k, o)  at bf16 element  (o / 128) * R32(K) * 128 + (k / 32) * 4096 + (o % 128 / 16) * 512
//                                     + ((k % 32 / 8) * 16 + o % 16) * 8 + k % 8
//     bias o         at word  bias + o                              (P(O) vectors of 128 floats, one per panel)
// padding rows, padding columns and padding biases are zero.  Matrices (off[] index; biases at off[15 + index]) are those of
// smz_mlp_layout_broad with R32(K) * 64 words per panel in the place of R8(K) * 128:
//     0 dyn_in, 1 ady_in     the hidden part, a panel matrix of K = S, O = H, then the action table [A][128 P(H)] bf16:
//                            element (a, o) at bf16 element a * 128 * P(H) + o behind word off + P(H) * R32(S) * 64
//     2 dyn_mid, 3 ady_mid, 8 pre_mid, 9 apr_mid, 13 rep_mid     panel matrices of K = H, O = H (absent when L = 0)
//     4 dyn_out              the reward logits, then the next state at off + P(S) * R32(H) * 64, biases at off[15 + 4] + 128 P(S)
//     5 ady_out, 14 rep_out  panel matrices of K = H, O = S
//     6 pre_in, 7 apr_in     panel matrices of K = S, O = H;  12 rep_in: K = obs, O = H
//     10 pre_out, 11 apr_out the policy, then the value at off + P(A) * R32(H) * 64, biases at off[15 + index] + 128 P(A)
// The representation matrices are packed in the same form; nothing here reads them.
// No descriptor of this layout equals one of smz_mlp_layout_broad: pre_in has the same size in both only for 9 <= S <= 16, and
// there dyn_in differs by A * P(H) * 64 words.
//
// Geometry: that of k_mlp_recurrent_broad -- workgroup (c, b) of four wavefronts takes the rows of branch b among the rows of
// chunk c; chunks of 16 rows up to B = 4096, of 32 rows above.  The switch is the float32 kernel's (no A/B of its own yet);
// SMZ_MLP_BROAD_BF16_SMALL_MAX replaces it.  A row's bits are the same in both.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/smz.h"
#include "smz_mlp_device.hpp"
#include "smz_mlp_wide_device.hpp"
#include "smz_mlp_broad_device.hpp"
#include "smz_mlp_broad_bf16_device.hpp"

using namespace smz_mlp;

namespace {

constexpr int kBf16Chunk = 2 * kTileLeaves;      // most rows per workgroup: at most one wavefront's lanes (the list comes from a ballot)

constexpr int kBf16SmallMax = 4096;              // largest batch in chunks of 16 rows (smz_mlp_recurrent_broad_bf16)

// CH = rows per chunk: kBf16Chunk (one or two tiles per workgroup) or kTileLeaves (one)
template <int CH>
__global__ void __launch_bounds__(kBroadWaves *kWave) k_mlp_recurrent_broad_bf16(smz_mlp_desc d, const float *__restrict__ image,
                                                                                 const float *__restrict__ parent_hidden,
                                                                                 const int32_t *__restrict__ last_action,
                                                                                 const uint8_t *__restrict__ branch,
                                                                                 float *__restrict__ hidden_out,
                                                                                 float *__restrict__ reward_out,
                                                                                 float *__restrict__ policy_out,
                                                                                 float *__restrict__ value_out, int B) {
    extern __shared__ uint4 bf16_tiles[];                // 2 x bf16_tile_vecs(S, H) uint4
    __shared__ BroadLds lds;
    uint4 *t0 = bf16_tiles, *t1 = t0 + bf16_tile_vecs(d.S, d.H);
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
        broad_bf16_tile(d, image, t0, t1, lds, count, ady, wave, lane,
                        [&](int lf, int k) { return parent_hidden[(base + li[lf]) * S + k]; },
                        [&](int lf) { return last_action[base + li[lf]]; },
                        [&](int lf) {
                            const size_t r = base + li[lf];
                            return WideDst{hidden_out + r * S, policy_out + r * A, value_out + r, reward_out + r};
                        });
    }
}

template <int CH>
int launch(const smz_mlp_desc *d, const void *weights_dev, const float *parent_hidden_dev, const int32_t *last_action_dev,
           const uint8_t *branch_dev, float *hidden_out_dev, float *reward_out_dev, float *policy_out_dev, float *value_out_dev, int B,
           smz_stream stream) {
    // two activation tiles: 2 KB (H <= 128, S <= 32) to 32 KB (H > 384), beside 2.4 KB of static LDS: within HIP's default limit
    const size_t lds = 2 * (size_t)bf16_tile_vecs(d->S, d->H) * sizeof(uint4);
    hipLaunchKernelGGL(k_mlp_recurrent_broad_bf16<CH>, dim3((B + CH - 1) / CH, 2), dim3(kBroadWaves * kWave), lds, (hipStream_t)stream,
                       *d, static_cast<const float *>(weights_dev), parent_hidden_dev, last_action_dev, branch_dev, hidden_out_dev,
                       reward_out_dev, policy_out_dev, value_out_dev, B);
    return hipGetLastError() == hipSuccess ? SMZ_OK : SMZ_ERR_HIP;
}

}  // namespace

extern "C" {

int smz_mlp_layout_broad_bf16(smz_mlp_desc *d) {
    if (!d || d->obs < 1 || d->A < 1 || d->S < 1 || d->H < 1 || d->L < 0) return SMZ_ERR_INVALID;
    if (d->A > SMZ_MAX_ACTIONS_LARGE || d->H > kBroadMaxH || d->S > kBroadMaxS) return SMZ_ERR_TOO_LARGE;
    d->OP = kWideOP;
    const int ph = broad_panels(d->H), ps = broad_panels(d->S), pa = broad_panels(d->A);
    const int wh = bf16_panel_words(d->H), ws = bf16_panel_words(d->S);    // words per panel of K = H, K = S
    const int mid = d->L > 0 ? ph * wh : 0, pmid = d->L > 0 ? ph : 0;      // one shared Linear(H, H) per trunk, applied L times
    const int in = ph * ws + d->A * ph * (kWideOP / 2);                    // hidden part + one table row of 128 P(H) bf16 per action
    // words per matrix, bias vectors of 128 floats per matrix (= its panels)
    const int words[M_COUNT] = {in, in, mid, mid, 2 * ps * wh, ps * wh, ph * ws, ph * ws, mid, mid, (pa + ps) * wh, (pa + ps) * wh,
                                ph * bf16_panel_words(d->obs), mid, ps * wh};
    const int vecs[M_COUNT] = {ph, ph, pmid, pmid, 2 * ps, ps, ph, ph, pmid, pmid, pa + ps, pa + ps, ph, pmid, ps};
    int off = 0;
    for (int m = 0; m < M_COUNT; m++) { d->off[m] = off; off += words[m]; }
    for (int m = 0; m < M_COUNT; m++) { d->off[M_COUNT + m] = off; off += vecs[m] * kWideOP; }
    d->total_floats = off;
    return SMZ_OK;
}

int smz_mlp_recurrent_broad_bf16(const smz_mlp_desc *d, const void *weights_dev, const float *parent_hidden_dev,
                                 const int32_t *last_action_dev, const uint8_t *branch_dev, float *hidden_out_dev,
                                 float *reward_out_dev, float *policy_out_dev, float *value_out_dev, int B, smz_stream stream) {
    if (!d || !weights_dev || !parent_hidden_dev || !last_action_dev || !branch_dev || !hidden_out_dev || !reward_out_dev ||
        !policy_out_dev || !value_out_dev || B < 1)
        return SMZ_ERR_INVALID;
    smz_mlp_desc t = *d;
    if (smz_mlp_layout_broad_bf16(&t) != SMZ_OK || t.total_floats != d->total_floats || d->OP != kWideOP) return SMZ_ERR_INVALID;
    for (int m = 0; m < 2 * M_COUNT; m++)
        if (t.off[m] != d->off[m]) return SMZ_ERR_INVALID;
    // chunks of 16 rows up to kBf16SmallMax rows, of 32 above (the header comment)
    int small_max = kBf16SmallMax;
    if (const char *e = getenv("SMZ_MLP_BROAD_BF16_SMALL_MAX")) small_max = atoi(e);     // (A/B runs: 0 = chunks of 32 rows always)
    return B <= small_max ? launch<kTileLeaves>(d, weights_dev, parent_hidden_dev, last_action_dev, branch_dev, hidden_out_dev,
                                                reward_out_dev, policy_out_dev, value_out_dev, B, stream)
                          : launch<kBf16Chunk>(d, weights_dev, parent_hidden_dev, last_action_dev, branch_dev, hidden_out_dev,
                                               reward_out_dev, policy_out_dev, value_out_dev, B, stream);
}

}  // extern "C"
