// smz_mlp_wide_search.hip -- the whole Monte_carlo_tree_search.run (mcts:311-349) of every tree in ONE launch for the wide
// `mlp_model` shapes (smz_mlp_layout_wide: H <= 128, 2 S <= 128, A + S <= 128 -- the reference's config 434 and its checkpoint
// 450): smz_search_mlp_wide / smz_search_mlp_wide_act.
//
// Step-wise, such a search is 1 + 2 x simulations launches, and every round carries mlp_input, branch, the hidden row, reward,
// policy and value through global memory between the tree kernel and k_mlp_recurrent_wide.  Here a workgroup of four wavefronts
// owns 4 x tpw trees for the whole search:
//   * tree phases (expand + backup of the previous leaf, select) one tree per lane, the per-lane device functions of the
//     step-wise kernels (smz_device.hpp); trees, hidden rows and path records stay in global memory in the handle's layout;
//   * the network phase once per round for the whole workgroup: every wavefront publishes its leaves to LDS, the leaves are
//     listed per branch, and the <= 16-leaf tiles are dealt round-robin to the four wavefronts.  A tile goes through wide_tile()
//     of smz_mlp_wide_device.hpp, the tile body of k_mlp_recurrent_wide, compiled with the same flags: inputs come straight from
//     the parent's hidden row and the action, the scaled hidden row goes straight into the new node's row, policy, value and
//     reward go to the tree's slot in LDS for the next round's expansion.  Weights are streamed from L2 as in the head kernel.
// A leaf's result does not depend on its tile mates (tests/test_gpu_mlp_envelope.py), so both paths compute the same search,
// bit for bit (tests/test_gpu_mlp_wide_search.py).
// Every wavefront of a workgroup reaches every barrier of every round: a wavefront without a searched tree stays in the loop
// and takes tiles; only a workgroup none of whose trees is searched leaves, as a whole, before the rounds start.
// The per-lane tree code needs every scalar register a wave has: the kernel's wave-uniform state is pinned or parked in vector
// registers (in_vgpr / unpark / pin_search_args of smz_search_frame.hpp, which also holds the pb_c staging and the tree's tail).
// Limits (anything else runs step-wise): one player, 2 or 4 actions, at most 64 trees per wavefront, LDS map <= 160 KB.
#include "smz_common.hpp"
#include "smz_handle.hpp"
#include "smz_mlp_wide_device.hpp"
#include "smz_search_frame.hpp"

using smz_mlp::kTileLeaves;
using smz_mlp::kWideOP;
using smz_mlp::kWideTileFloats;
using smz_mlp::lds_sync;
using smz_mlp::WideDst;

namespace {

constexpr int kWgPerCu = 1;                  // workgroups the geometry puts on a CU before a wave takes a second tree (register-bound: see DESIGN.md 3.6)
constexpr int kSearchWaves = 4;              // wavefronts per workgroup

// LDS map (float offsets from the dynamic LDS base): four activation tiles | leaf records [4 tpw] int4 (tree, leaf, parent,
// action) | leaf lists [2][4 tpw] uint16 | counts [4][2] + flags [4] | pb_c table + reciprocals (doubles) | head outputs
// [4 tpw][A + 2] (policy | value | reward) | per wave: rng tile [tpw][kRngStride]
struct WideLds {
    int recs, list, cnt, pbc, outs, wave, per_wave, total;
};
__host__ __device__ inline WideLds wide_lds(int A, int sims, int tpw) {
    WideLds m;
    const int slots = kSearchWaves * tpw;
    m.recs = kSearchWaves * kWideTileFloats;
    m.list = m.recs + 4 * slots;
    m.cnt = m.list + r4((2 * slots + 1) / 2);
    m.pbc = m.cnt + 12;
    m.outs = m.pbc + r4(2 * 2 * (sims + 2));
    m.wave = m.outs + r4(slots * (A + 2));
    m.per_wave = r4(tpw * kRngStride);
    m.total = m.wave + kSearchWaves * m.per_wave;
    return m;
}

extern __shared__ float4 smz_wsearch_lds4[];

// KS: children per expansion as the step-wise kernels compile it (2: the static two-child block code; 0: run-time K)
template <int MAXA, bool PHX = false, int KS = 0>
__global__ void __launch_bounds__(kSearchWaves *kWave, kWgPerCu) k_search_mlp_wide(Params Pin, smz_mlp_desc d, const float *__restrict__ weights,
                                                                                   const float *__restrict__ hidden0,
                                                                                   const float *__restrict__ policy0, int train, ActOut act) {
    Params P = Pin;
    P.tree0 = 0;
    P.philox = PHX ? 1 : 0;                  // (a constant in everything inlined below)
    // the action count equals its bucket (the entry point refuses anything else): the per-action arrays of the tree code stay
    // in registers instead of scratch memory
    P.A = MAXA;
    if (KS > 0) P.K = KS;
    fix_layout(P, true, KS > 0);
    float *lds = reinterpret_cast<float *>(smz_wsearch_lds4);
    pin_search_args(P, act, KS > 0);
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int A = P.A, S = P.S, tpw = P.tpw, sims = P.sims;
    const WideLds ml = wide_lds(A, sims, tpw);
    P.S = in_vgpr(P.S); P.sims = in_vgpr(P.sims); P.B = in_vgpr(P.B); P.active = in_vgpr(P.active);
    const int slots = kSearchWaves * tpw;
    int4 *recs = reinterpret_cast<int4 *>(lds + in_vgpr(ml.recs));
    unsigned short *list = reinterpret_cast<unsigned short *>(lds + in_vgpr(ml.list));
    int *cnt = reinterpret_cast<int *>(lds + in_vgpr(ml.cnt)), *flags = cnt + 2 * kSearchWaves;
    double *pbc_lds = reinterpret_cast<double *>(lds + in_vgpr(ml.pbc));
    float *outs_all = lds + in_vgpr(ml.outs);
    float *tile = lds + wave * kWideTileFloats;
    uint32_t *rng_tile = reinterpret_cast<uint32_t *>(lds + in_vgpr(ml.wave + wave * ml.per_wave));
    __builtin_assume(rng_tile != nullptr);                       // (the staging helpers test it: as a vector value that test is a lane mask kept for the whole search)
    const int ow = A + 2;
    const int sl = in_vgpr(wave * tpw + lane);                   // this lane's tree slot of the workgroup (lane < tpw)
    float *outs = outs_all + sl * ow;

    const int tree0 = in_vgpr((int)(blockIdx.x * kSearchWaves + wave) * tpw);
    const int tree = tree0 + lane;
    // (an int in a vector register, compared where it is used: as a bool it would be a lane mask in a scalar register pair for the whole search)
    const int valid_v = in_vgpr((lane < tpw && tree < P.B && tree_active(P, tree)) ? 1 : 0);
#define valid (fresh(valid_v) != 0)
    // parked (see unpark): trees per wave | hidden size | rounds | 1 = this wave owns a searched tree
    const int tpw_v = in_vgpr(tpw), S_v = in_vgpr(S), sims_v = in_vgpr(sims);
    const unsigned long long vmask = __ballot(valid);
    const int on_v = in_vgpr(vmask != 0ull ? 1 : 0);
    const int first_v = in_vgpr(vmask != 0ull ? (int)__builtin_ctzll(vmask) : 0);

    // ---- one-time staging: the pb_c table and its reciprocals; does the workgroup search anything? -------------------------
    stage_pbc(pbc_lds, P, sims);
    if (lane == 0) flags[wave] = vmask != 0ull ? 1 : 0;
    __syncthreads();
    // every tree of the workgroup switched off (smz_set_active): all four wavefronts leave here, before the rounds' barriers
    if ((flags[0] | flags[1] | flags[2] | flags[3]) == 0) return;

    // ---- root: hidden state and policy come from the heads' initial() ------------------------------------------------------
    RngT<PHX> rng;
    TreeHdr h = {};
    int packed = 0;
    if (unpark(on_v) != 0) {                                     // (wave-uniform)
        const int ntw = unpark(tpw_v);
        for (int t = 0; t < ntw; t++) {
            if (((vmask >> t) & 1ull) == 0) continue;
            const int row = tree0 + t;
            for (int k = lane; k < S; k += kWave) P.hidden[(size_t)row * P.N * P.hs + k] = hidden0[(size_t)row * S + k];
            if (lane < A) outs_all[(wave * ntw + t) * ow + lane] = policy0[(size_t)row * A + lane];
        }
        lds_sync();
        packed = wave_stage_rng<PHX>(P, tree, valid, rng_tile);
        // The root expansion runs in EVERY lane of such a wave, without a branch on `valid`: a lane that owns no searched tree
        // repeats the work of the wave's first searched slot -- same tree, same staged words, same stream position, in lock step
        // with that lane, so it stores the same values to the same addresses and its own results are never read
        // (smz_lstm_search.hip: the execution mask an `if (valid)` around root_init_tree would keep is a scalar register pair
        // that no longer fits).
        const int first = unpark(first_v);
        const int lane_m = valid ? lane : first, tree_m = tree0 + lane_m;
        const int packed_first = __builtin_amdgcn_readlane(packed, first);
        packed = valid ? packed : packed_first;
        rng.bind(P, tree_m, true);
        rng.load(P.mt + (size_t)tree_m * kMtN, packed, rng_tile + lane_m * kRngStride, kRngStage);
        P.sims = unpark(sims_v);            // (root_init_tree branches on it: a uniform branch, no saved execution mask)
        root_init_tree<MAXA>(P, tree_m, rng, outs_all + (wave * ntw + lane_m) * ow, nullptr, train != 0);
        P.sims = sims_v;
        h = P.hdr[tree_m];
        packed = rng.pack();
        // random words are staged once per round, for the NEXT round
        P.tpw = ntw;
        if (unpark(sims_v) > 0) packed = wave_stage_rng_from<4, PHX>(P, tree, valid, rng_tile, packed, rng.block());
    }
    unsigned n_dec = 0, n_chance = 0, n_children = 0;

    // ---- simulations: three workgroup barriers per round, reached by all four wavefronts ------------------------------------
    for (int s_v = in_vgpr(0); unpark(s_v) < unpark(sims_v); s_v++) {
        Leaf L = {0, 0, 0, 0};
        if (valid) {
            rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + lane * kRngStride, kRngStage);
            if (s_v > 0) expand_backup_tree<MAXA, KS>(P, tree, rng, h, outs, outs[A + 1], outs[A], path_col(P, tree));
            int len = 0;
            L = select_tree<MAXA, KS, false, true>(P, tree, rng, h, pbc_lds, len, n_dec, n_chance, n_children, path_col(P, tree));
            h.path_len = len;
            packed = rng.pack();
        }
        // publish this wave's leaves: the record of every searched tree, and how many leaves of each branch the wave has
        const bool dyn = valid && L.branch != 0, ady = valid && L.branch == 0;
        const unsigned long long m_dyn = __ballot(dyn), m_ady = __ballot(ady);
        if (valid) recs[sl] = make_int4(tree, L.leaf_id, L.parent_id, L.action);
        if (lane == 0) { cnt[2 * wave] = __popcll(m_dyn); cnt[2 * wave + 1] = __popcll(m_ady); }
        __syncthreads();                                                                                   // (1) counts
        // lists per branch in wave order, a wave's leaves in lane order (the order is fixed, though no result depends on it)
        int n0 = 0, n1 = 0, off0 = 0, off1 = 0;
#pragma unroll
        for (int w = 0; w < kSearchWaves; w++) {
            const int c0 = cnt[2 * w], c1 = cnt[2 * w + 1];
            if (w < wave) { off0 += c0; off1 += c1; }
            n0 += c0; n1 += c1;
        }
        n0 = __builtin_amdgcn_readfirstlane(n0); n1 = __builtin_amdgcn_readfirstlane(n1);
        {
            const unsigned long long below = (1ull << lane) - 1ull;
            const int nsl = unpark(tpw_v) * kSearchWaves;
            if (dyn) list[off0 + __popcll(m_dyn & below)] = (unsigned short)sl;
            if (ady) list[nsl + off1 + __popcll(m_ady & below)] = (unsigned short)sl;
        }
        __syncthreads();                                                                                   // (2) lists, records
        {
            const int nsl = unpark(tpw_v) * kSearchWaves, Sr = unpark(S_v);
            const int t0 = (n0 + kTileLeaves - 1) / kTileLeaves, t1 = (n1 + kTileLeaves - 1) / kTileLeaves;
            for (int tl = wave; tl < t0 + t1; tl += kSearchWaves) {
                const bool tady = tl >= t0;                                  // wave-uniform
                const int tt = tady ? tl - t0 : tl, count = (tady ? n1 : n0) - tt * kTileLeaves;
                const unsigned short *li = list + (tady ? nsl : 0) + tt * kTileLeaves;
                // inputs: the parent's hidden row + the one-hot action (what k_select writes to mlp_input); outputs: the new
                // node's row of the handle's hidden array and the tree's slot of head outputs
                smz_mlp::wide_tile(d, weights, tile, count, tady, lane,
                                   [&](int lf, int k) {
                                       const int4 r = recs[li[lf]];
                                       return k < Sr ? P.hidden[((size_t)r.x * P.N + r.z) * P.hs + k] : ((k - Sr) == r.w ? 1.f : 0.f);
                                   },
                                   [&](int lf) {
                                       const int s = li[lf];
                                       const int4 r = recs[s];
                                       float *o = outs_all + s * ow;
                                       return WideDst{P.hidden + ((size_t)r.x * P.N + r.y) * P.hs, o, o + A, o + A + 1};
                                   });
            }
        }
        // a tile wave wrote hidden rows (global) and head outputs (LDS) of trees other waves own: rows a later round reads as
        // parent rows, outputs the next expansion reads.  Workgroup-scope release / acquire around the barrier.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();                                                                                   // (3) results
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (unpark(on_v) != 0) {
            P.tpw = unpark(tpw_v);
            packed = wave_stage_rng_from<4, PHX>(P, tree, valid, rng_tile, packed, rng.block());
        }
    }
    if (valid)
        finish_tree<MAXA, KS>(P, tree, rng, h, packed, sims_v, rng_tile + lane * kRngStride, outs, A, path_col(P, tree), act);
#undef valid
}

int search_mlp_wide_launch(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *hidden0_dev,
                           const float *policy0_dev, int train, ActOut act, const double *pow_table_host, smz_stream stream) {
    if (h && h->large_actions) return refuse_large_actions("smz_search_mlp_wide");
    if (!h || !desc || !weights_dev || !hidden0_dev || !policy0_dev) return fail(SMZ_ERR_INVALID, "smz_search_mlp_wide: null argument%s");
    if (h->P.n_cycle > 1) return refuse_multi_player("smz_search_mlp_wide");
    {
        smz_mlp_desc t = *desc;
        if (smz_mlp_layout_wide(&t) != SMZ_OK || t.total_floats != desc->total_floats || desc->OP != kWideOP)
            return fail(SMZ_ERR_INVALID, "smz_search_mlp_wide: descriptor does not describe a wide mlp_model weight buffer (smz_mlp_layout_wide)%s");
    }
    if (desc->A != h->P.A || desc->S != h->P.S)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_wide: network dimensions differ from the handle's%s");
    if (h->maxa > 4 || h->P.A != h->maxa)
        return fail(SMZ_ERR_TOO_LARGE, "smz_search_mlp_wide: outside the single-launch kernel's limits (2 or 4 actions): use the step-wise entry points%s");
    if (const int rc = check_dirichlet_alpha(h, train)) return rc;
    DeviceGuard guard(h->cfg.device);
    Params P = h->P;
    // kWgPerCu workgroups of four wavefronts on each CU before a wave takes a second tree
    const int tpw = single_launch_tpw(P.B, kWgPerCu * kCus * kSearchWaves, "SMZ_WIDE_SEARCH_TPW");
    const WideLds ml = wide_lds(P.A, P.sims, tpw);
    if (const int rc = check_single_launch_size("smz_search_mlp_wide", tpw, ml.total)) return rc;
    const size_t lds = (size_t)ml.total * sizeof(float);
    if (act.action && use_pow_table(h, P, act.temperature, pow_table_host, stream) != SMZ_OK) return SMZ_ERR_HIP;
    P.tpw = tpw;
    const int blocks = (P.B + kSearchWaves * tpw - 1) / (kSearchWaves * tpw), ks = h->K == 2 ? 2 : 0;
#define SMZ_LAUNCH_WS(MA, KK) (P.philox ? SMZ_LAUNCH_WS1(MA, true, KK) : SMZ_LAUNCH_WS1(MA, false, KK))
#define SMZ_LAUNCH_WS1(MA, PX, KK)                                                                                     \
    launch_with_lds<k_search_mlp_wide<MA, PX, KK>>(h, blocks, kSearchWaves * kWave, lds, stream, P, *desc, weights_dev, hidden0_dev, \
                                                   policy0_dev, train, act)
    const int rc = h->maxa == 2 ? (ks ? SMZ_LAUNCH_WS(2, 2) : SMZ_LAUNCH_WS(2, 0)) : (ks ? SMZ_LAUNCH_WS(4, 2) : SMZ_LAUNCH_WS(4, 0));
#undef SMZ_LAUNCH_WS
#undef SMZ_LAUNCH_WS1
    if (rc != SMZ_OK) return rc;
    // (the name as rocprofv3 prints it: without the defaulted arguments)
    if (ks) snprintf(h->last_kernel, sizeof(h->last_kernel), "k_search_mlp_wide<%d, %s, %d>", h->maxa, P.philox ? "true" : "false", ks);
    else snprintf(h->last_kernel, sizeof(h->last_kernel), P.philox ? "k_search_mlp_wide<%d, true>" : "k_search_mlp_wide<%d>", h->maxa);
    return search_launched(h);
}

}  // namespace

extern "C" {

int smz_search_mlp_wide(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *hidden0_dev,
                        const float *policy0_dev, int train, smz_stream stream) {
    return search_mlp_wide_launch(h, desc, weights_dev, hidden0_dev, policy0_dev, train, kNoAct, nullptr, stream);
}

int smz_search_mlp_wide_act(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *hidden0_dev,
                            const float *policy0_dev, int train, double temperature, const double *pow_table_host,
                            int32_t *action_dev, double *policy_dev, double *child_visits_dev, float *root_value_dev,
                            smz_stream stream) {
    if (const int rc = check_act_outputs("smz_search_mlp_wide_act", action_dev, policy_dev, child_visits_dev)) return rc;
    return search_mlp_wide_launch(h, desc, weights_dev, hidden0_dev, policy0_dev, train,
                                  ActOut{temperature, action_dev, policy_dev, child_visits_dev, root_value_dev}, pow_table_host, stream);
}

}  // extern "C"
