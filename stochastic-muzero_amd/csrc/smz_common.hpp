// smz_common.hpp -- what every tree translation unit of libsmz.so sees: the tuning switches and their defaults, the device
// headers, and the wave-cooperative helpers (random-word staging, hidden-row moves) shared by the step-wise kernels, the
// single-launch searches and the built-in env.  Everything with internal linkage: each unit inlines its own copy.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no FMA contraction: parity with the reference's
// separately rounded multiplies and adds).
#pragma once
#ifndef SMZ_SEARCH_THREADS
#define SMZ_SEARCH_THREADS 512   // threads per workgroup the single-launch search is register-allocated for (8 waves: 2 per SIMD, 256 VGPRs)
#endif
#ifndef SMZ_EB_WAVES
#define SMZ_EB_WAVES 4   // waves per SIMD the step-wise tree kernels are register-allocated for
#endif
#ifndef SMZ_PAIR_K4
#define SMZ_PAIR_K4 1              // KS = 4: the paired descent on every decision level (0: one lane scores all four children)
#endif
#ifndef SMZ_KS4
#define SMZ_KS4 1                  // the compile-time K = 4 instantiation for the A = 4 bucket (0: run-time K as in round 5)
#endif
// Wave priorities inside the search kernel (s_setprio): the network evaluation is throughput work, the tree phases are
// dependent chains that mostly wait; letting the evaluating wave of a SIMD issue first measured +4 % (392 -> 408 M
// simulations/s, same box, back to back; every non-uniform assignment tried beat uniform priorities).
#ifndef SMZ_PRIO_TREE
#define SMZ_PRIO_TREE 0
#define SMZ_PRIO_HEADS 3
#endif
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <algorithm>
#include <vector>

#include "../../include/smz.h"
#include "smz_device.hpp"
#include "smz_mlp_device.hpp"
#include "smz_select_masks.hpp"

using namespace smz;

// (file scope, not the anonymous namespace: it crosses translation units by value)
struct EnvStep {
    double *state;                 // [B][4] f64 in/out; nullptr: no env step in this launch
    float *obs_out, *reward_out;
    uint8_t *flag_out;
    int32_t *step_count, *episode; // nullptr: no bookkeeping (plain step: flag = terminated)
    uint8_t *active;
    int limit, on_end;
    uint64_t reset_seed;
    long long first_env;
    double *traj;                  // [T][B][13] f64 or nullptr
    int t;
};

namespace {

struct RowGeom {  // how the 64 lanes of a wave are split over rows of `width` floats
    int width, lpr, rows_per_iter;
};

__host__ __device__ inline RowGeom row_geom(int width) {
    int lpr = 1;
    while (lpr < width && lpr < kWave) lpr <<= 1;
    RowGeom g;
    g.width = width;
    g.lpr = lpr;
    g.rows_per_iter = kWave / lpr;
    return g;
}

// Value of lane 0 or lane 1 (src = 0 / 1, may differ per lane): two v_readlane and a select instead of a ds_bpermute round
// trip (~120 cycles in the middle of the tree phases' dependent chains).
__device__ inline int pick_lane01(int v, int src) {
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 1);
    return src ? b : a;
}
__device__ inline float pick_lane01(float v, int src) { return __int_as_float(pick_lane01(__float_as_int(v), src)); }
__device__ inline uint64_t readlane64(uint64_t v, int l) {        // (l: wave-uniform)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// Random-word staging: for each of the wave's 64 trees, all 64 lanes cooperate on that tree's NEXT 64 words --
// lane j owns word (idx + j) mod 624; words not yet twisted (j >= ready) are twisted in place (every lane reads
// its three source words before any lane stores, which is exactly the sequential in-place order because the
// sources of word p are p, p+1 and p+397 and at most 64 consecutive words change) -- and the tempered words go to
// this wave's LDS tile [tree lane][word].  Global traffic is coalesced 256-byte segments.  Returns the lane's
// packed (ready << 16 | idx) after staging.
// Philox mode: the next words of the wave's trees are computed, not loaded -- lanes 0..15 of tree slot t evaluate the 16
// counter blocks that cover words [idx & ~3, (idx & ~3) + 64) of its stream and write those at or after idx to the tile
// row (Rng::load knows the row then holds 64 - (idx & 3) words).  `block`: each lane's own tree's block counter.
__device__ inline void philox_stage(const Params &P, int tree, bool valid, uint32_t *lds_tile, int packed, uint32_t block, int ntrees) {
    if (!lds_tile) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int tree0 = tree - lane;
    for (int t0 = 0; t0 < ntrees; t0 += 4) {                      // four trees per pass: 16 lanes each
        const int t = t0 + (lane >> 4), j = lane & 15;
        const int src = t < ntrees ? t : 0;
        const int pk = __shfl(packed, src);
        const uint32_t kb = (uint32_t)__shfl((int)block, src);
        const bool vt = t < ntrees && __shfl((int)valid, src) != 0;
        if (vt) {
            const int idx = pk & 0xffff;
            int q = (idx >> 2) + j;
            uint32_t b = kb;
            if (q >= kMtN / 4) { q -= kMtN / 4; ++b; }
            const uint64_t n = (uint64_t)b * (kMtN / 4) + (uint64_t)q;
            const PhiloxOut o = philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), P.rng_key[2 * (tree0 + t)], P.rng_key[2 * (tree0 + t) + 1]);
            const int pos = 4 * j - (idx & 3);
            uint32_t *row = lds_tile + t * kRngStride;
            if (pos >= 0) row[pos] = o.x;
            if (pos + 1 >= 0) row[pos + 1] = o.y;
            if (pos + 2 >= 0) row[pos + 2] = o.z;
            row[pos + 3] = o.w;
        }
    }
}

template <int U = 8, bool PHC = true>   // U trees in flight: their loads are all issued before the first dependent store
__device__ inline int wave_stage_rng_from(const Params &P, int tree, bool valid, uint32_t *lds_tile, int packed, uint32_t block = 0u) {
    const int lane = threadIdx.x & (kWave - 1);
    const int tree0 = tree - lane;
    if constexpr (PHC) {
        if (P.philox) {
            philox_stage(P, tree, valid, lds_tile, packed, block, P.tpw);
            return ((kRngStage) << 16) | (packed & 0xffff);
        }
    }
    for (int t0 = 0; t0 < P.tpw; t0 += U) {
        uint32_t w[U], b[U], c[U];
        int pos[U];
        bool tw[U], vt[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int pk = __shfl(packed, t0 + u);
            vt[u] = __shfl((int)valid, t0 + u) != 0;          // wave-uniform
            const int idx = pk & 0xffff, ready = pk >> 16;
            const uint32_t *mt = P.mt + (size_t)(tree0 + t0 + u) * kMtN;
            int p = idx + lane;
            if (p >= kMtN) p -= kMtN;
            pos[u] = p;
            tw[u] = vt[u] && lane >= ready;
            w[u] = b[u] = c[u] = 0u;
            if (vt[u]) w[u] = mt[p];
            if (tw[u]) {
                const int p1 = (p + 1 == kMtN) ? 0 : p + 1;
                int pm = p + kMtM;
                if (pm >= kMtN) pm -= kMtN;
                b[u] = mt[p1];
                c[u] = mt[pm];
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (tw[u]) {
                w[u] = mt_twist(w[u], b[u], c[u]);
                (P.mt + (size_t)(tree0 + t0 + u) * kMtN)[pos[u]] = w[u];
            }
            if (vt[u] && lds_tile) lds_tile[(t0 + u) * kRngStride + lane] = mt_temper(w[u]);
        }
    }
    const int idx = packed & 0xffff, ready = packed >> 16;
    return ((ready > kRngStage ? ready : kRngStage) << 16) | idx;
}

// Half-width staging for wavefronts of 16+ trees (mid-size and large batches, MT19937): 32 words per tree and launch instead of 64 -- a
// simulation draws ~10 (the rare longer one falls back to the words in global memory, same values) -- two trees per pass, lanes
// 0..31 | 32..63.  At a million trees the 64-word window alone was 4-5 of the ~10 cache lines a tree reads per launch.
#ifndef SMZ_RNG_NARROW
#define SMZ_RNG_NARROW 32
#endif
constexpr int kRngStageNarrow = SMZ_RNG_NARROW;      // 16 or 32
__device__ inline int wave_stage_rng_narrow(const Params &P, int tree, bool valid, uint32_t *lds_tile) {
    constexpr int U = 8;
    constexpr int W = kRngStageNarrow, TP = kWave / W;      // trees per pass
    const int lane = threadIdx.x & (kWave - 1), half = lane / W, j = lane % W;
    const int tree0 = tree - lane;
    const int packed = valid ? P.rng_pos[tree] : 0;
    for (int t0 = 0; t0 < P.tpw; t0 += TP * U) {
        uint32_t w[U], b[U], c[U];
        int pos[U];
        bool tw[U], vt[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = t0 + TP * u + half;
            const int pk = __shfl(packed, t);
            vt[u] = __shfl((int)valid, t) != 0;
            const int idx = pk & 0xffff, ready = pk >> 16;
            const uint32_t *mt = P.mt + (size_t)(tree0 + t) * kMtN;
            int p = idx + j;
            if (p >= kMtN) p -= kMtN;
            pos[u] = p;
            tw[u] = vt[u] && j >= ready;
            w[u] = b[u] = c[u] = 0u;
            if (vt[u]) w[u] = mt[p];
            if (tw[u]) {
                const int p1 = (p + 1 == kMtN) ? 0 : p + 1;
                int pm = p + kMtM;
                if (pm >= kMtN) pm -= kMtN;
                b[u] = mt[p1];
                c[u] = mt[pm];
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = t0 + TP * u + half;
            if (tw[u]) {
                w[u] = mt_twist(w[u], b[u], c[u]);
                (P.mt + (size_t)(tree0 + t) * kMtN)[pos[u]] = w[u];
            }
            if (vt[u]) lds_tile[t * kRngStride + j] = mt_temper(w[u]);
        }
    }
    const int idx = packed & 0xffff, ready = packed >> 16;
    return ((ready > kRngStageNarrow ? ready : kRngStageNarrow) << 16) | idx;
}

template <bool PHC = true>
__device__ inline int wave_stage_rng(const Params &P, int tree, bool valid, uint32_t *lds_tile) {
    return wave_stage_rng_from<8, PHC>(P, tree, valid, lds_tile, valid ? P.rng_pos[tree] : 0,
                                       (PHC && P.philox && valid) ? P.rng_block[tree] : 0u);
}

// SMZ_STAGE_STORES_LAST (round 5): stage_finish stores the twisted words after ALL trees' words went to LDS (=0: tree by tree).
#ifndef SMZ_STAGE_STORES_LAST
#define SMZ_STAGE_STORES_LAST 1
#endif
// The same staging split in two for waves that own at most U trees: stage_issue requests the source words (the loads
// stay in flight while the caller does unrelated work -- the network evaluation in k_search_mlp), stage_finish twists,
// stores and fills the LDS tile.  Nothing may draw random words of these trees in between.
template <int U>
struct StagePre {
    uint32_t w[U], b[U], c[U];
};
template <int U, bool PHC = true>
__device__ inline void stage_issue(const Params &P, int tree, bool valid, int packed, StagePre<U> &pre) {
    const int lane = threadIdx.x & (kWave - 1);
    const int tree0 = tree - lane;
    if (PHC && P.philox) return;                            // nothing to load: stage_finish computes the words
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int pk = __builtin_amdgcn_readlane(packed, u);              // (u is a constant after unrolling)
        const bool vt = u < P.tpw && __builtin_amdgcn_readlane((int)valid, u) != 0;          // wave-uniform
        const int idx = pk & 0xffff, ready = pk >> 16;
        const uint32_t *mt = P.mt + (size_t)(tree0 + u) * kMtN;
        int p = idx + lane;
        if (p >= kMtN) p -= kMtN;
        pre.w[u] = pre.b[u] = pre.c[u] = 0u;
        if (vt) pre.w[u] = mt[p];
        if (vt && lane >= ready) {
            const int p1 = (p + 1 == kMtN) ? 0 : p + 1;
            int pm = p + kMtM;
            if (pm >= kMtN) pm -= kMtN;
            pre.b[u] = mt[p1];
            pre.c[u] = mt[pm];
        }
    }
}
template <int U, bool PHC = true>
__device__ inline int stage_finish(const Params &P, int tree, bool valid, uint32_t *lds_tile, int packed, const StagePre<U> &pre,
                                   uint32_t block = 0u) {
    const int lane = threadIdx.x & (kWave - 1);
    const int tree0 = tree - lane;
    if constexpr (PHC) {
        if (P.philox) {
            philox_stage(P, tree, valid, lds_tile, packed, block, P.tpw < U ? P.tpw : U);
            return ((kRngStage) << 16) | (packed & 0xffff);
        }
    }
#if SMZ_STAGE_STORES_LAST
    // Every source word is consumed (twisted, tempered, handed to LDS) before the first twisted word is stored: a store between
    // one tree's words and the next's made the compiler wait for THAT STORE's completion (vmcnt counts stores on gfx9, and with
    // the twist under a branch its count is conservative: s_waitcnt vmcnt(0) after each global_store -- two serial store round
    // trips per round, profiles/r05_s_stage_waits.txt).
    uint32_t tw_w[U];
    int tw_p[U];
    bool tw_on[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int pk = __builtin_amdgcn_readlane(packed, u);
        const bool vt = u < P.tpw && __builtin_amdgcn_readlane((int)valid, u) != 0;
        const int idx = pk & 0xffff, ready = pk >> 16;
        int p = idx + lane;
        if (p >= kMtN) p -= kMtN;
        tw_on[u] = vt && lane >= ready;
        tw_p[u] = p;
        const uint32_t t = mt_twist(pre.w[u], pre.b[u], pre.c[u]);      // (lanes that do not twist hold zeros in b, c: value unused)
        tw_w[u] = tw_on[u] ? t : pre.w[u];
        if (vt) lds_tile[u * kRngStride + lane] = mt_temper(tw_w[u]);
    }
#pragma unroll
    for (int u = 0; u < U; u++)
        if (tw_on[u]) (P.mt + (size_t)(tree0 + u) * kMtN)[tw_p[u]] = tw_w[u];
#else
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int pk = __builtin_amdgcn_readlane(packed, u);
        const bool vt = u < P.tpw && __builtin_amdgcn_readlane((int)valid, u) != 0;
        const int idx = pk & 0xffff, ready = pk >> 16;
        int p = idx + lane;
        if (p >= kMtN) p -= kMtN;
        uint32_t w = pre.w[u];
        if (vt && lane >= ready) {
            w = mt_twist(w, pre.b[u], pre.c[u]);
            (P.mt + (size_t)(tree0 + u) * kMtN)[p] = w;
        }
        if (vt) lds_tile[u * kRngStride + lane] = mt_temper(w);
    }
#endif
    const int idx = packed & 0xffff, ready = packed >> 16;
    return ((ready > kRngStage ? ready : kRngStage) << 16) | idx;
}

// Row moves.  `lpr` consecutive lanes move one row of `width` floats; the rows of the wave's 64 trees are handed
// around with ds_bpermute.  Loads of kRowBatch rows are issued before the first store so that the (independent)
// row reads overlap instead of each waiting behind the previous row's may-alias store.
constexpr int kRowBatch = 8;

// Moves one row per tree of this wave.  src_row/dst_row are per-lane row pointers (of the lane's own tree).
// Every lane executes every shuffle (a lane whose column index falls outside the row still serves as a source).
__device__ inline void wave_copy_rows(const float *src_row, float *dst_row, bool valid, int width, int tpw) {
    const RowGeom g = row_geom(width);
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane / g.lpr, li = lane % g.lpr;
    const unsigned long long s64 = (unsigned long long)src_row, d64 = (unsigned long long)dst_row;
    const int iters = (tpw + g.rows_per_iter - 1) / g.rows_per_iter;
    for (int it0 = 0; it0 < iters; it0 += kRowBatch) {
        unsigned long long sj[kRowBatch], dj[kRowBatch];
        bool ok[kRowBatch];
#pragma unroll
        for (int u = 0; u < kRowBatch; u++) {
            const int it = it0 + u;
            const int j = ((it < iters ? it : 0) * g.rows_per_iter + sub) & (kWave - 1);
            sj[u] = __shfl(s64, j);
            dj[u] = __shfl(d64, j);
            ok[u] = (it < iters) && (__shfl((int)valid, j) != 0);
        }
        for (int i = li; i < width; i += g.lpr) {                   // one pass per lpr-wide column slab
            float v[kRowBatch];
#pragma unroll
            for (int u = 0; u < kRowBatch; u++) v[u] = ok[u] ? ((const float *)sj[u])[i] : 0.f;
#pragma unroll
            for (int u = 0; u < kRowBatch; u++)
                if (ok[u]) ((float *)dj[u])[i] = v[u];
        }
    }
}

// Network-input gather of smz_select: parent hidden rows (+ one-hot of the last action) for the wave's 64 trees.
__device__ inline void wave_gather_inputs(const Params &P, int tree, bool valid, int parent, int act,
                                          float *parent_hidden, float *mlp_input) {
    const int S = P.S, W = S + P.A;
    const RowGeom g = row_geom(mlp_input ? W : S);
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane / g.lpr, li = lane % g.lpr;
    const int tree0 = tree - lane;
    const int iters = (P.tpw + g.rows_per_iter - 1) / g.rows_per_iter;
    for (int it0 = 0; it0 < iters; it0 += kRowBatch) {
        int tj[kRowBatch], pj[kRowBatch], aj[kRowBatch];
        bool ok[kRowBatch];
#pragma unroll
        for (int u = 0; u < kRowBatch; u++) {
            const int it = it0 + u;
            const int j = ((it < iters ? it : 0) * g.rows_per_iter + sub) & (kWave - 1);
            pj[u] = __shfl(parent, j);
            aj[u] = __shfl(act, j);
            ok[u] = (it < iters) && (__shfl((int)valid, j) != 0);
            tj[u] = tree0 + j;
        }
        for (int i = li; i < g.width; i += g.lpr) {
            float v[kRowBatch];
#pragma unroll
            for (int u = 0; u < kRowBatch; u++) {
                v[u] = 0.f;
                if (ok[u]) v[u] = (i < S) ? P.hidden[((size_t)tj[u] * P.N + pj[u]) * P.hs + i] : ((i - S) == aj[u] ? 1.0f : 0.0f);
            }
#pragma unroll
            for (int u = 0; u < kRowBatch; u++) {
                if (ok[u]) {
                    if (mlp_input) mlp_input[(size_t)tj[u] * W + i] = v[u];
                    if (parent_hidden && i < S) parent_hidden[(size_t)tj[u] * S + i] = v[u];
                }
            }
        }
    }
}

__device__ inline void wave_add_stats(unsigned long long *stats, unsigned a, unsigned b, unsigned c, unsigned d) {
    if (!stats) return;
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
        c += __shfl_down(c, off);
        d += __shfl_down(d, off);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicAdd(&stats[0], (unsigned long long)a);
        atomicAdd(&stats[1], (unsigned long long)b);
        atomicAdd(&stats[2], (unsigned long long)c);
        atomicAdd(&stats[3], (unsigned long long)d);
    }
}

// sqrt(n) * pb_c(n) table staged in LDS (dynamic shared memory) when it fits, so that the pUCT loop does not pay a
// dependent global load per level.
constexpr int kPbcLdsMax = 4096;
extern __shared__ double smz_dyn_lds[];
__device__ inline const double *stage_pbc(const Params &P) {
    const int n = P.sims + 2;
    if (n > kPbcLdsMax) return P.pbc_sqrt;
    for (int i = threadIdx.x; i < n; i += kWave) smz_dyn_lds[i] = P.pbc_sqrt[i];
    __syncthreads();
    return smz_dyn_lds;
}
// dynamic LDS of the step-wise tree kernels: [pbc table (when it fits)] [rng tile (when P.lds_stage)]
__device__ inline uint32_t *rng_tile_ptr(const Params &P) {
    if (!P.lds_stage) return nullptr;
    const int n = (P.sims + 2 <= kPbcLdsMax) ? P.sims + 2 : 0;
    return reinterpret_cast<uint32_t *>(smz_dyn_lds + n);
}

// (always inlined: with the multi-player kernels beside them, the wide buckets' fused kernels would otherwise call it)
template <int MAXA, int KS, class RNG>
__device__ __forceinline__ void select_phase(const Params &P, int tree, bool valid, RNG &rng, TreeHdr &h, const double *pbc_lds,
                                             float *parent_hidden, int32_t *last_action, uint8_t *branch, float *mlp_input) {
    Leaf L = {0, 0, 0, 0};
    unsigned n_dec = 0, n_chance = 0, n_children = 0;
    if (valid) {
        int len = 0;
        L = select_tree<MAXA, KS, true, false, false>(P, tree, rng, h, pbc_lds, len, n_dec, n_chance, n_children, path_col(P, tree));
        h.path_len = len;
        if (last_action) last_action[tree] = L.action;
        if (branch) branch[tree] = (uint8_t)L.branch;
    }
    if (P.ids_out && (int)threadIdx.x < P.tpw && tree < P.B) {
        P.ids_out[2 * (size_t)tree] = valid ? L.leaf_id : -1;
        P.ids_out[2 * (size_t)tree + 1] = valid ? L.parent_id : -1;
    }
    if (P.S > 0 && (parent_hidden || mlp_input))
        wave_gather_inputs(P, tree, valid, L.parent_id, L.action, parent_hidden, mlp_input);
    wave_add_stats(P.stats, n_dec, n_chance, valid ? 1u : 0u, n_children);
}

// Block geometry as a function of A and K (the formulas of smz_create): with compile-time A / K these fold to constants.
__device__ inline void fix_layout(Params &P, bool a_const, bool k_const) {
    if (a_const) { P.rp_off = (5 * P.A + 1) & ~1; P.rb_words = ((P.rp_off + 2 * P.A) + 15) & ~15; }
    if (k_const) P.eb_words = ((6 * P.K) + 15) & ~15;
}

// Counter-based generator of the built-in environments (reset states of later episodes, stand-in observations):
// splitmix64 of (seed, env, episode / step, component) -- the same value whatever the shard or launch geometry.
__host__ __device__ inline uint64_t smz_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline double smz_unit(uint64_t seed, uint64_t env, uint64_t epoch, uint64_t comp) {   // [0, 1)
    const uint64_t z = smz_mix64(smz_mix64(smz_mix64(seed ^ (env * 0xD1342543DE82EF95ull)) + epoch) + comp);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// One env step of the built-in CartPole-v1 shaped env + its trajectory record (k_traj_pack's layout, A = 2), with the game
// bookkeeping of self_play.py:79 / game.py:270-271 -- the ONE body behind smz_cartpole_step, _step_pack, _step_ctl and
// the tail of the single-launch search (smz_search_mlp_act_cartpole).  The flag written to flag_out / the record's
// `terminated` slot is 0 running, 1 terminated (Game.done True), 2 stopped by limit_of_game_play (the game is over but
// Game.done stays False, game.py:270-271), 3 no step taken (env switched off).  on_end: 1 = a finished env is switched off
// (active[e] = 0: the searches skip it from now on), 2 = it starts its next episode at once (state ~ U(-0.05, 0.05)^4 from
// the counter-based generator, episode[e] + 1).
__device__ inline void cartpole_env_step(const EnvStep &E, int e, int B, const int32_t *action, const double *policy,
                                         const double *child_visits, const float *root_value) {
    constexpr int A = 2, F = 4 + 3 * A + 3;
    double *r = E.traj ? E.traj + ((size_t)E.t * B + e) * F : nullptr;
    if (E.active && !E.active[e]) {
        if (E.flag_out) E.flag_out[e] = 3;
        if (E.reward_out) E.reward_out[e] = 0.f;
        if (r) { for (int k = 0; k < F; k++) r[k] = 0.0; r[5] = 3.0; }
        return;
    }
    const double g = 9.8, mc = 1.0, mp = 0.1, tm = mc + mp, len = 0.5, pml = mp * len, fm = 10.0, tau = 0.02;
    double *st = E.state + (size_t)e * 4;
    const double x = st[0], xd = st[1], th = st[2], thd = st[3];
    const int act = action[e];
    const double force = act == 1 ? fm : -fm;
    const double ct = cos(th), sn = sin(th);
    const double temp = (force + pml * thd * thd * sn) / tm;
    const double tha = (g * sn - ct * temp) / (len * (4.0 / 3.0 - mp * ct * ct / tm));
    const double xa = temp - pml * tha * ct / tm;
    double nx = x + tau * xd, nxd = xd + tau * xa, nth = th + tau * thd, nthd = thd + tau * tha;
    const bool term = fabs(nx) > 2.4 || fabs(nth) > 12.0 * 2.0 * 3.14159265358979323846 / 360.0;
    const int count = E.step_count ? E.step_count[e] + 1 : 0;
    const int flag = (E.limit > 0 && count == E.limit) ? 2 : (term ? 1 : 0);
    if (r) {
        r[0] = (double)(float)nx; r[1] = (double)(float)nxd; r[2] = (double)(float)nth; r[3] = (double)(float)nthd;
        r[4] = 1.0;
        r[5] = (double)flag;
        r[6] = policy[(size_t)e * A]; r[7] = policy[(size_t)e * A + 1];
        r[8] = act == 0 ? 1.0 : 0.0; r[9] = act == 1 ? 1.0 : 0.0;
        r[10] = (double)root_value[e];
        r[11] = child_visits[(size_t)e * A]; r[12] = child_visits[(size_t)e * A + 1];
    }
    if (E.reward_out) E.reward_out[e] = 1.0f;
    if (E.flag_out) E.flag_out[e] = (uint8_t)flag;
    int next_count = count;
    if (flag != 0 && E.on_end == 2) {
        const int ep = E.episode[e] + 1;
        E.episode[e] = ep;
        nx = -0.05 + 0.1 * smz_unit(E.reset_seed, (uint64_t)(E.first_env + e), (uint64_t)ep, 0);
        nxd = -0.05 + 0.1 * smz_unit(E.reset_seed, (uint64_t)(E.first_env + e), (uint64_t)ep, 1);
        nth = -0.05 + 0.1 * smz_unit(E.reset_seed, (uint64_t)(E.first_env + e), (uint64_t)ep, 2);
        nthd = -0.05 + 0.1 * smz_unit(E.reset_seed, (uint64_t)(E.first_env + e), (uint64_t)ep, 3);
        next_count = 0;
    } else if (flag != 0 && E.on_end == 1 && E.active) {
        E.active[e] = 0;
    }
    if (E.step_count) E.step_count[e] = next_count;
    st[0] = nx; st[1] = nxd; st[2] = nth; st[3] = nthd;
    if (E.obs_out) {
        float *o = E.obs_out + (size_t)e * 4;
        o[0] = (float)nx; o[1] = (float)nxd; o[2] = (float)nth; o[3] = (float)nthd;
    }
}

constexpr int kCus = 256;    // MI355X: the compute units the single-launch searches spread their workgroups over

// (LDS maps of the single-launch searches: every part padded to 16 bytes)
__host__ __device__ inline int r4(int x) { return (x + 3) & ~3; }

struct ActOut {              // smz_search_mlp_act: Game.policy_step folded into the tail of the launch (action == nullptr: off)
    double temperature;
    int32_t *action;
    double *policy, *child_visits;
    float *root_value;
};

}  // namespace
