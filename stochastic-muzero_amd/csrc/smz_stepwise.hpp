// smz_stepwise.hpp -- the step-wise tree kernels (one search tree per lane, one 64-lane wavefront per workgroup): templates
// instantiated by smz_kernels.hip (smz_root_init, smz_select, smz_expand_backup) and smz_fused.hip (smz_expand_backup_select).
#pragma once
#include "smz_common.hpp"

namespace {

template <int MAXA>
__global__ void __launch_bounds__(kWave) k_root_init(Params P, const float *hidden, const float *policy,
                                                     const double *noise_override, int train) {
    uint32_t *rng_tile = rng_tile_ptr(P);
    const int n_staged = rng_tile ? kRngStage : 0;
    const int tree = blockIdx.x * P.tpw + threadIdx.x;
    const bool valid = (int)threadIdx.x < P.tpw && tree < P.B && tree_active(P, tree);
    const int packed = wave_stage_rng(P, tree, valid, rng_tile);
    if (valid) {
        Rng rng;
        rng.bind(P, tree, valid);
        rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + threadIdx.x * kRngStride, n_staged);
        root_init_tree<MAXA>(P, tree, rng, policy + (size_t)tree * P.A,
                             noise_override ? noise_override + (size_t)tree * P.A : nullptr, train != 0);
        P.rng_pos[tree] = rng.pack();
        rng.save(P, tree);
    }
    if (P.S > 0 && hidden) {
        const int t = valid ? tree : 0;
        wave_copy_rows(hidden + (size_t)t * P.S, P.hidden + (size_t)t * P.N * P.hs, valid, P.S, P.tpw);
    }
}

// AEX (instantiated for the MAXA 2 and 4 buckets): the action count equals the bucket, so A (and K when KS > 0) are
// compile-time constants in everything inlined below (see k_search_mlp).
template <int MAXA, int KS, bool AEX>
__global__ void __launch_bounds__(kWave, 4) k_select(Params Pin, float *parent_hidden, int32_t *last_action,
                                                  uint8_t *branch, float *mlp_input) {
    Params P = Pin;
    P.tree0 = 0;
    if (AEX) P.A = MAXA;
    if (KS > 0) P.K = KS;
    fix_layout(P, AEX, KS > 0);
    uint32_t *rng_tile = rng_tile_ptr(P);
    const bool narrow = rng_tile && P.tpw >= 16 && !P.philox;          // (wave-uniform) 16+ trees per wavefront: wave_stage_rng_narrow
    const int n_staged = rng_tile ? (narrow ? kRngStageNarrow : kRngStage) : 0;
    const int tree = blockIdx.x * P.tpw + threadIdx.x;
    const bool valid = (int)threadIdx.x < P.tpw && tree < P.B && tree_active(P, tree);
    const double *pbc_lds = stage_pbc(P);
    const int packed = narrow ? wave_stage_rng_narrow(P, tree, valid, rng_tile) : wave_stage_rng<!AEX>(P, tree, valid, rng_tile);
    RngT<!AEX> rng;          // (the specialised instantiations serve MT19937 handles only: see smz_select)
    rng.bind(P, tree, valid);
    TreeHdr h = {0, 0, 0.f, 0.f, 0, 0.f, 0, 0};
    if (valid) {
        rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + threadIdx.x * kRngStride, n_staged);
        h = P.hdr[tree];
    }
    select_phase<MAXA, KS>(P, tree, valid, rng, h, pbc_lds, parent_hidden, last_action, branch, mlp_input);
    if (valid) {
        P.rng_pos[tree] = rng.pack();
        rng.save(P, tree);
        P.hdr[tree] = h;
    }
}

// PHX (round 5, with AEX): the specialised kernel for Philox handles -- counter streams, no MT19937 state to load, twist or store
template <int MAXA, int KS, bool FUSE_SELECT, bool AEX, bool PHX = false>
__global__ void __launch_bounds__(kWave, MAXA > 16 ? 1 : SMZ_EB_WAVES) k_expand_backup(Params Pin, const float *hidden, const float *reward,
                                                         const float *policy, const float *value,
                                                         float *parent_hidden, int32_t *last_action, uint8_t *branch,
                                                         float *mlp_input) {
    Params P = Pin;
    P.tree0 = 0;
    if (AEX) P.A = MAXA;
    if (AEX) P.philox = PHX ? 1 : 0;          // (a constant in everything inlined below)
    if (KS > 0) P.K = KS;
    fix_layout(P, AEX, KS > 0);
    uint32_t *rng_tile = rng_tile_ptr(P);
    const bool narrow = rng_tile && P.tpw >= 16 && !P.philox;          // (wave-uniform) 16+ trees per wavefront: wave_stage_rng_narrow
    const int n_staged = rng_tile ? (narrow ? kRngStageNarrow : kRngStage) : 0;
    const int tree = blockIdx.x * P.tpw + threadIdx.x;
    const bool valid = (int)threadIdx.x < P.tpw && tree < P.B && tree_active(P, tree);
    const double *pbc_lds = stage_pbc(P);
    const int packed = narrow ? wave_stage_rng_narrow(P, tree, valid, rng_tile) : wave_stage_rng<!AEX || PHX>(P, tree, valid, rng_tile);
    RngT<!AEX || PHX> rng;
    rng.bind(P, tree, valid);
    TreeHdr h = {0, 0, 0.f, 0.f, 0, 0.f, 0, 0};
    int leaf = 0;
    if (valid) {
        rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + threadIdx.x * kRngStride, n_staged);
        h = P.hdr[tree];
        leaf = expand_backup_tree<MAXA, KS>(P, tree, rng, h, policy + (size_t)tree * P.A, reward ? reward[tree] : 0.0f,
                                            value[tree], path_col(P, tree));
    }
    if (P.S > 0 && hidden) {
        const int t = valid ? tree : 0;
        wave_copy_rows(hidden + (size_t)t * P.S, P.hidden + ((size_t)t * P.N + leaf) * P.hs, valid, P.S, P.tpw);
    }
    if (FUSE_SELECT) {
        // the leaf rows just written by other lanes of this wave may be the next parent rows
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        select_phase<MAXA, KS>(P, tree, valid, rng, h, pbc_lds, parent_hidden, last_action, branch, mlp_input);
    }
    if (valid) {
        P.rng_pos[tree] = rng.pack();
        rng.save(P, tree);
        P.hdr[tree] = h;
    }
}
// The same kernel with the multi-player backup (smz_set_players: value_sum gains -value at the nodes of the root's opponents).
// A kernel of its own, so that k_expand_backup keeps its instruction stream.
template <int MAXA, int KS, bool FUSE_SELECT, bool AEX, bool PHX = false>
__global__ void __launch_bounds__(kWave, MAXA > 16 ? 1 : SMZ_EB_WAVES) k_expand_backup_mp(Params Pin, const float *hidden, const float *reward,
                                                            const float *policy, const float *value,
                                                            float *parent_hidden, int32_t *last_action, uint8_t *branch,
                                                            float *mlp_input) {
    Params P = Pin;
    P.tree0 = 0;
    if (AEX) P.A = MAXA;
    if (AEX) P.philox = PHX ? 1 : 0;          // (a constant in everything inlined below)
    if (KS > 0) P.K = KS;
    fix_layout(P, AEX, KS > 0);
    uint32_t *rng_tile = rng_tile_ptr(P);
    const bool narrow = rng_tile && P.tpw >= 16 && !P.philox;          // (wave-uniform) 16+ trees per wavefront: wave_stage_rng_narrow
    const int n_staged = rng_tile ? (narrow ? kRngStageNarrow : kRngStage) : 0;
    const int tree = blockIdx.x * P.tpw + threadIdx.x;
    const bool valid = (int)threadIdx.x < P.tpw && tree < P.B && tree_active(P, tree);
    const double *pbc_lds = stage_pbc(P);
    const int packed = narrow ? wave_stage_rng_narrow(P, tree, valid, rng_tile) : wave_stage_rng<!AEX || PHX>(P, tree, valid, rng_tile);
    RngT<!AEX || PHX> rng;
    rng.bind(P, tree, valid);
    TreeHdr h = {0, 0, 0.f, 0.f, 0, 0.f, 0, 0};
    int leaf = 0;
    if (valid) {
        rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + threadIdx.x * kRngStride, n_staged);
        h = P.hdr[tree];
        leaf = expand_backup_tree<MAXA, KS, false, false, false, true>(P, tree, rng, h, policy + (size_t)tree * P.A,
                                                                     reward ? reward[tree] : 0.0f, value[tree], path_col(P, tree));
    }
    if (P.S > 0 && hidden) {
        const int t = valid ? tree : 0;
        wave_copy_rows(hidden + (size_t)t * P.S, P.hidden + ((size_t)t * P.N + leaf) * P.hs, valid, P.S, P.tpw);
    }
    if (FUSE_SELECT) {
        // the leaf rows just written by other lanes of this wave may be the next parent rows
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        select_phase<MAXA, KS>(P, tree, valid, rng, h, pbc_lds, parent_hidden, last_action, branch, mlp_input);
    }
    if (valid) {
        P.rng_pos[tree] = rng.pack();
        rng.save(P, tree);
        P.hdr[tree] = h;
    }
}

}  // namespace
