// smz_mlp_players_search.hip -- the whole Monte_carlo_tree_search.run (mcts:311-349) of every tree of a MULTI-PLAYER handle
// (smz_set_players: number_of_player > 1 or a custom loop) in ONE launch, for the `mlp_model` networks smz_mlp_layout accepts
// (LDS-resident; HipMlpHeads): smz_search_mlp_players / smz_search_mlp_players_act.
//
// Step-wise, such a search is 1 + 2 x simulations launches, and every round carries mlp_input, branch, the hidden row, reward,
// policy and value through global memory.  smz_search_mlp refuses a multi-player handle; this kernel is the generic path of
// k_search_mlp (trees in global memory, run-time A <= MAXA, masks honoured) with the signed backup:
//   * one staging per workgroup: the networks without the representation matrices (stage_weights_without_rep), the pb_c table
//     and its reciprocals.  One workgroup barrier ends the staging; none follows, so a wavefront without a searched tree
//     (beyond B, or all of its trees switched off with smz_set_active) simply returns;
//   * a wavefront owns `tpw` trees for the whole search.  Tree phases run one tree per lane with the per-lane device functions
//     of the step-wise kernels (smz_device.hpp): expand_backup_tree<..., MP = true>, as k_expand_backup_mp calls it, and
//     select_tree.  The sign mask, the turn index and root_player[tree] % n_cycle all come from that shared function: there is
//     no multi-player code in this file;
//   * the network phase row by row by the whole wavefront: smz_mlp::initial_row at the root, smz_mlp::recurrent_rows in the
//     rounds -- the row bodies of the HipMlpHeads kernels, compiled with the same flags.  The scaled hidden row goes straight
//     into the new node's row of the handle's hidden array; policy, value and reward go to the tree's slot in LDS for the next
//     round's expansion.  Random words are staged once per round, for the next round;
//   * path records live in LDS, [tpw][P] uint4 per wavefront (1,664 B per wavefront at 4096 x 50); the last path is copied to
//     the handle's level-major array at the end, where the debug dump expects it.
// Both paths draw the same random words and round alike: the searches are bit-identical (tests/test_gpu_mlp_players_search.py).
//
// Geometry: workgroups of eight wavefronts, one per CU (the weight image alone is ~100 KB at the checkpoint-421 shape), so 2048
// wavefronts have a tree each before any takes a second one: tpw = ceil(B / 2048), at most 64.  SMZ_PLAYERS_SEARCH_TPW overrides
// it (tests: a search does not depend on the geometry).
// Limits (anything else runs step-wise): at most 32 actions, at most 64 trees per wavefront, LDS map <= 160 KB, no statistics.
#include "smz_common.hpp"
#include "smz_handle.hpp"
#include "smz_search_frame.hpp"

using smz_mlp::lds_sync;
using smz_mlp::up4;

namespace {

constexpr int kPlayersWaves = 8;             // wavefronts per workgroup (SMZ_SEARCH_THREADS: 2 per SIMD, 256 VGPRs each)
static_assert(kPlayersWaves * kWave == SMZ_SEARCH_THREADS, "register-allocated like k_search_mlp");

// LDS map (float offsets from the dynamic LDS base): networks without the representation matrices | pb_c table + reciprocals
// (doubles) | per wave, every part padded to 16 bytes: one row's scratch | network inputs [tpw][up4(S + A)] | path records
// [tpw][P] uint4 | rng tile [tpw][kRngStride] | head outputs [tpw][A + 2] (policy | value | reward)
struct PlayersLds {
    int pbc, wave, per_wave, x, pv, rng, outs;
    long long total;
};
__host__ __device__ inline PlayersLds players_lds(const smz_mlp_desc &d, const Params &P, int tpw) {
    PlayersLds m;
    m.pbc = r4(d.total_floats - smz_mlp::rep_floats(d));
    m.wave = m.pbc + r4(2 * 2 * (P.sims + 2));
    m.x = r4(smz_mlp::scratch_floats(d));
    m.pv = m.x + tpw * up4(P.S + P.A);
    m.rng = m.pv + tpw * P.P * 4;
    m.outs = m.rng + r4(tpw * kRngStride);
    m.per_wave = m.outs + r4(tpw * (P.A + 2));
    m.total = (long long)m.wave + (long long)kPlayersWaves * m.per_wave;
    return m;
}

extern __shared__ float4 smz_psearch_lds4[];

// KS: children per expansion as the step-wise kernels compile it (2: the static two-child block code; 0: run-time K)
template <int MAXA, int KS, bool PHX>
__global__ void __launch_bounds__(SMZ_SEARCH_THREADS) k_search_mlp_players(Params Pin, smz_mlp_desc d, const float *weights, const float *obs,
                                                                            int train, ActOut act) {
    Params P = Pin;
    P.tree0 = 0;
    P.philox = PHX ? 1 : 0;                  // (a constant in everything inlined below)
    if (KS > 0) P.K = KS;
    fix_layout(P, false, KS > 0);
    float *lds = reinterpret_cast<float *>(smz_psearch_lds4);
    // ---- one-time staging: everything but the representation matrices, the pb_c table and its reciprocals -------------------
    const smz_mlp_desc dl = smz_mlp::lds_desc_without_rep(d);
    smz_mlp::stage_weights_without_rep(lds, weights, d);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int A = P.A, S = P.S, tpw = P.tpw;
    const PlayersLds ml = players_lds(d, P, tpw);
    double *pbc_lds = reinterpret_cast<double *>(lds + ml.pbc);
    stage_pbc(pbc_lds, P, P.sims);
    const int slot = A + 2;
    const int K4in = up4(S + A);
    float *scratch = lds + ml.wave + wave * ml.per_wave;
    float *xall = scratch + ml.x;                                               // [tpw][K4in] network inputs of the round
    uint4 *pvals = reinterpret_cast<uint4 *>(scratch + ml.pv);                  // [tpw][P] path records
    uint32_t *rng_tile = reinterpret_cast<uint32_t *>(scratch + ml.rng);
    float *outs = scratch + ml.outs;                                            // [tpw][A + 2]: policy | value | reward
    __syncthreads();                         // the only workgroup barrier of the kernel

    const int tree0 = (blockIdx.x * kPlayersWaves + wave) * tpw;
    const int tree = tree0 + lane;
    const bool valid = lane < tpw && tree < P.B && tree_active(P, tree);
    // a wave none of whose trees is searched (beyond B, or switched off with smz_set_active) is done
    if (__ballot(valid) == 0ull) return;

    // ---- root: representation + prediction per row, then root expansion per lane ---------------------------------------------
    for (int t = 0; t < tpw; t++) {
        const int row = tree0 + t;
        if (row >= P.B) break;                                   // wave-uniform
        if (!__shfl((int)valid, t)) continue;                    // wave-uniform: the tree is switched off
        smz_mlp::initial_row<1, false>(lds, dl, weights, d, scratch, obs + (size_t)row * d.obs, P.hidden + (size_t)row * P.N * P.hs,
                                       nullptr, outs + t * slot);
    }
    int packed = wave_stage_rng<PHX>(P, tree, valid, rng_tile);
    RngT<PHX> rng;
    rng.bind(P, tree, valid);
    TreeHdr h = {0, 0, 0.f, 0.f, 0, 0.f, 0, 0};
    if (valid) {
        rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + lane * kRngStride, kRngStage);
        root_init_tree<MAXA>(P, tree, rng, outs + lane * slot, nullptr, train != 0);
        h = P.hdr[tree];
        packed = rng.pack();
    }
    unsigned n_dec = 0, n_chance = 0, n_children = 0;
    // random words are staged once per round, for the NEXT round
    if (P.sims > 0) packed = wave_stage_rng_from<4, PHX>(P, tree, valid, rng_tile, packed, rng.block());

    // ---- simulations --------------------------------------------------------------------------------------------------------
    for (int s = 0; s < P.sims; s++) {
        Leaf L = {0, 0, 0, 0};
        if (valid) {
            rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + lane * kRngStride, kRngStage);
            // the multi-player backup, as k_expand_backup_mp calls it
            if (s > 0) expand_backup_tree<MAXA, KS, false, false, false, /*MP=*/true>(P, tree, rng, h, outs + lane * slot, outs[lane * slot + A + 1],
                                                                                   outs[lane * slot + A], pvals + lane * P.P);
            int len = 0;
            L = select_tree<MAXA, KS, false, true>(P, tree, rng, h, pbc_lds, len, n_dec, n_chance, n_children, pvals + lane * P.P);
            h.path_len = len;
            packed = rng.pack();
        }
        // hidden rows written in earlier rounds (by any lane of this wave) may be this round's parent rows
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        // all rows' network inputs first (independent global loads, one latency), then the rows one after another
        for (int t = 0; t < tpw; t++) {
            const int row = tree0 + t;
            if (row >= P.B) break;                               // wave-uniform
            const int parent = __builtin_amdgcn_readlane(L.parent_id, t), actn = __builtin_amdgcn_readlane(L.action, t);
            const float *src = P.hidden + ((size_t)row * P.N + parent) * P.hs;
            for (int k = lane; k < K4in; k += kWave)
                xall[t * K4in + k] = (k < S) ? src[k] : ((k < S + A && (k - S) == actn) ? 1.f : 0.f);
        }
        lds_sync();
        for (int t = 0; t < tpw; t++) {
            const int row = tree0 + t;
            if (row >= P.B) break;                               // wave-uniform
            if (!__shfl((int)valid, t)) continue;                // a switched-off tree: no network pass
            const float *xin[1] = {xall + t * K4in};
            const bool dyn[1] = {__builtin_amdgcn_readlane(L.branch, t) != 0}, live[1] = {true};
            float *dh[1] = {P.hidden + ((size_t)row * P.N + __builtin_amdgcn_readlane(L.leaf_id, t)) * P.hs}, *dp[1] = {outs + t * slot};
            float reward[1], value[1];
            smz_mlp::recurrent_rows<1, smz_mlp::kRows, false, false>(lds, dl, scratch, xin, dyn, live, dh, dp, reward, value);
            if (lane == 0) { outs[t * slot + A] = value[0]; outs[t * slot + A + 1] = reward[0]; }
        }
        lds_sync();
        packed = wave_stage_rng_from<4, PHX>(P, tree, valid, rng_tile, packed, rng.block());
    }
    // ---- tail: the last expansion + backup, header, stream position, (act) ----------------------------------------------------
    if (valid) {
        if (P.sims > 0) {
            rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + lane * kRngStride, kRngStage);
            expand_backup_tree<MAXA, KS, false, false, false, /*MP=*/true>(P, tree, rng, h, outs + lane * slot, outs[lane * slot + A + 1],
                                                                        outs[lane * slot + A], pvals + lane * P.P);
            // leave the last path where the step-wise entry points and the debug dump expect it
            for (int i = 0; i < h.path_len; i++) P.path[(size_t)i * P.B + tree] = pvals[lane * P.P + i];
            packed = rng.pack();
        }
        P.hdr[tree] = h;
        if (act.action) {
            // the post-search policy / action of game.py:179-232 on the finished tree: the same draws from the same stream
            // position as a separate smz_act launch (rng still holds this tree's position)
            act_tree<MAXA>(P, tree, rng, act.temperature, act.action, act.policy, act.child_visits, act.root_value);
            packed = rng.pack();
        }
        P.rng_pos[tree] = packed;
        rng.save(P, tree);
    }
}

int search_mlp_players_launch(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev, int train,
                              ActOut act, const double *pow_table_host, smz_stream stream) {
    if (h && h->large_actions) return refuse_large_actions("smz_search_mlp_players");
    if (!h || !desc || !weights_dev || !obs_dev) return fail(SMZ_ERR_INVALID, "smz_search_mlp_players: null argument%s");
    if (h->P.n_cycle <= 1)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_players: a one-player handle (smz_set_players with more than one cycle entry selects this kernel): use smz_search_mlp%s");
    if (h->P.stats || h->P.dbg)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_players: no instrumented variant (smz_enable_stats / SMZ_DEBUG_SKIP): use the step-wise entry points%s");
    {
        smz_mlp_desc t = *desc;
        if (smz_mlp_layout(&t) != SMZ_OK || t.total_floats != desc->total_floats)
            return fail(SMZ_ERR_INVALID, "smz_search_mlp_players: descriptor does not describe an LDS-resident network%s");
    }
    if (desc->A != h->P.A || desc->S != h->P.S)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_players: network dimensions differ from the handle's%s");
    if (const int rc = check_dirichlet_alpha(h, train)) return rc;
    DeviceGuard guard(h->cfg.device);
    Params P = h->P;
    // one workgroup of eight wavefronts on each CU before a wave takes a second tree
    const int tpw = single_launch_tpw(P.B, kCus * kPlayersWaves, "SMZ_PLAYERS_SEARCH_TPW");
    const PlayersLds ml = players_lds(*desc, P, tpw);
    if (const int rc = check_single_launch_size("smz_search_mlp_players", tpw, ml.total)) return rc;
    const size_t lds = (size_t)ml.total * sizeof(float);
    if (act.action && use_pow_table(h, P, act.temperature, pow_table_host, stream) != SMZ_OK) return SMZ_ERR_HIP;
    P.tpw = tpw;
    const int blocks = (P.B + kPlayersWaves * tpw - 1) / (kPlayersWaves * tpw), ks = h->K == 2 ? 2 : 0;
#define SMZ_LAUNCH_PS(MA) (ks ? SMZ_LAUNCH_PS1(MA, 2) : SMZ_LAUNCH_PS1(MA, 0))
#define SMZ_LAUNCH_PS1(MA, KK) (P.philox ? SMZ_LAUNCH_PS2(MA, KK, true) : SMZ_LAUNCH_PS2(MA, KK, false))
#define SMZ_LAUNCH_PS2(MA, KK, PX)                                                                                     \
    launch_with_lds<k_search_mlp_players<MA, KK, PX>>(h, blocks, kPlayersWaves * kWave, lds, stream, P, *desc, weights_dev, obs_dev, \
                                                      train, act)
    int rc;
    switch (h->maxa) {
        case 2: rc = SMZ_LAUNCH_PS(2); break;
        case 4: rc = SMZ_LAUNCH_PS(4); break;
        case 8: rc = SMZ_LAUNCH_PS(8); break;
        case 16: rc = SMZ_LAUNCH_PS(16); break;
        default: rc = SMZ_LAUNCH_PS(32); break;
    }
#undef SMZ_LAUNCH_PS
#undef SMZ_LAUNCH_PS1
#undef SMZ_LAUNCH_PS2
    if (rc != SMZ_OK) return rc;
    snprintf(h->last_kernel, sizeof(h->last_kernel), "k_search_mlp_players<%d, %d, %s>", h->maxa, ks, P.philox ? "true" : "false");
    return search_launched(h);
}

}  // namespace

extern "C" {

int smz_search_mlp_players(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev, int train,
                           smz_stream stream) {
    return search_mlp_players_launch(h, desc, weights_dev, obs_dev, train, kNoAct, nullptr, stream);
}

int smz_search_mlp_players_act(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev, int train,
                               double temperature, const double *pow_table_host, int32_t *action_dev, double *policy_dev,
                               double *child_visits_dev, float *root_value_dev, smz_stream stream) {
    if (const int rc = check_act_outputs("smz_search_mlp_players_act", action_dev, policy_dev, child_visits_dev)) return rc;
    return search_mlp_players_launch(h, desc, weights_dev, obs_dev, train,
                                     ActOut{temperature, action_dev, policy_dev, child_visits_dev, root_value_dev}, pow_table_host, stream);
}

}  // extern "C"
