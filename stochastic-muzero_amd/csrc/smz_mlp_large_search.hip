// smz_mlp_large_search.hip -- the rounds of a whole Monte_carlo_tree_search.run (mcts:311-349) in ONE launch for large-action
// handles (smz_create_large_actions: 1 <= A <= SMZ_MAX_ACTIONS_LARGE) whose networks are the large-action `mlp_model` image
// (smz_mlp_layout_large): smz_search_mlp_large / smz_search_mlp_large_act.
//
// Step-wise, a round of such a search is three launches (k_select_la, k_mlp_recurrent_large[_split], k_expand_backup_la), and
// parent rows, actions, branches, hidden rows, rewards, policies and values travel through global memory between them; every
// tree kernel loads and stores its tree's MT19937 state.  Here the launcher issues the step-wise root kernels (k_root_init_la,
// then k_root_noise_la when training), ONE k_search_mlp_large for all num_simulations rounds, and k_act_la when asked for an action.
//
// k_search_mlp_large: a workgroup of kLargeWaves = 4 wavefronts owns T trees (1 <= T <= 4: ceil(B / 256), a workgroup on every CU
// before any takes a second tree, at most what large_search_lds fits into 160 KB), wavefront w < T owns tree blockIdx.x * T + w
// for the whole search -- a wavefront per tree, as the step-wise kernels.
//   * tree phases: la_select_tree and la_expand_backup_tree of smz_large_actions_device.hpp, the bodies of the step-wise kernels,
//     on the wavefront's own LaLds area.  The generator is loaded before round 0 and saved after the last expansion; the MT19937
//     words stay in LDS in between.  Select publishes its leaf (parent row, action, branch, leaf node id, or "none") to LDS.
//   * network phase, once per round, all four wavefronts: every wavefront lists the <= T leaves per branch in wave order
//     (dynamics first, then afterstate) and, for a non-empty branch, calls large_tile<4> of smz_mlp_large_device.hpp -- the tile
//     body of k_mlp_recurrent_large_split, compiled with the same flags.  Inputs come straight from the parent's hidden row and
//     the recorded action; the scaled hidden row goes straight into the new node's row; value and reward go to the tree's slot
//     in LDS; the policy (and, before it, the parked logits) goes to the tree's row of the handle's policy work rows [B][A] in
//     global memory (4 x 1024 floats do not fit LDS beside the trees).
// Barriers: every wavefront of a workgroup executes both workgroup barriers of every round and the barriers inside
// large_tile<4> -- also a wavefront that owns no tree or a switched-off one: it publishes "none" and takes its panels.  The round
// count is uniform.  A workgroup none of whose trees is searched leaves as a whole before the first round.  Four wavefronts write
// different panels of a policy row and the owning wavefront reads all of it in the next tree phase: workgroup-scope release /
// acquire fences stand around the barrier between them, and the reads are ordinary loads.
// Bits: a leaf's outputs depend neither on its tile mates nor on its place in the tile, and the tree code is the step-wise
// code, so trees, root statistics, hidden rows and stream positions equal the step-wise search bit for bit wherever that runs
// k_mlp_recurrent_large_split (up to 2048 trees at A <= 128, up to 4096 above).  Beyond that the step-wise head kernel sums the
// panels in another order (PARTS = 1) and policies may differ in their last float32 bits.
// Limits: one player; anything else is refused.  Build: the flags of every unit (-ffp-contract=off).
#include "smz_common.hpp"
#include "smz_handle.hpp"
#include "smz_large_actions_device.hpp"
#include "smz_mlp_large_device.hpp"

using smz_mlp::kLargeWaves;
using smz_mlp::kTileLeaves;
using smz_mlp::kWideOP;
using smz_mlp::kWideTileFloats;
using smz_mlp::lds_sync;
using smz_mlp::M_COUNT;
using smz_mlp::WideDst;

namespace {

constexpr int kLargeSearchLdsMax = 160 * 1024;

// LDS map (byte offsets from the dynamic LDS base): four activation tiles | xw [4][16][2] floats | leaf records [4] int4
// (parent node, action, branch, leaf node or -1 = none) | (value, reward) [4] | searched flags [4] | per wavefront: leaf lists
// [2][4] int | T per-tree areas of la_lds_bytes(A).  The small parts have a slot per WAVEFRONT (a wavefront without a tree
// publishes "none").  T: the `want` trees the launcher asks for, at most the largest count whose map fits a CU's 160 KB
// (T = 0: not even one fits).  The launcher and the kernel call this one function with the same arguments.
struct LargeSearchLds {
    int xw, recs, vr, flags, lists, trees, per_tree, T, total;
};
__host__ __device__ inline LargeSearchLds large_search_lds(int A, int want) {
    LargeSearchLds m;
    m.xw = kLargeWaves * kWideTileFloats * 4;
    m.recs = m.xw + kLargeWaves * kTileLeaves * 2 * 4;
    m.vr = m.recs + kLargeWaves * 16;
    m.flags = m.vr + kLargeWaves * 8;
    m.lists = m.flags + kLargeWaves * 4;
    m.trees = m.lists + kLargeWaves * 2 * kLargeWaves * 4;
    m.per_tree = (int)la_lds_bytes(A);
    m.T = (kLargeSearchLdsMax - m.trees) / m.per_tree;
    if (m.T > kLargeWaves) m.T = kLargeWaves;
    if (m.T < 0) m.T = 0;
    if (want >= 1 && want < m.T) m.T = want;
    m.total = m.trees + m.T * m.per_tree;
    return m;
}
static_assert(kLargeWaves * kWideTileFloats * 4 % 16 == 0, "the per-tree areas start on 16 bytes");

template <bool PHX>
__global__ void __launch_bounds__(kLargeWaves *kWave) k_search_mlp_large(Params P, smz_mlp_desc d, const float *__restrict__ weights,
                                                                        float *policy_work) {
    char *lds = reinterpret_cast<char *>(smz_dyn_lds);
    const int lane = la_lane(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int A = P.A, sims = P.sims;
    const LargeSearchLds m = large_search_lds(A, P.tpw);          // (P.tpw: the launcher's `want`)
    float *tile = reinterpret_cast<float *>(lds) + wave * kWideTileFloats;
    float *xw = reinterpret_cast<float *>(lds + m.xw);
    int4 *recs = reinterpret_cast<int4 *>(lds + m.recs);
    float *vr = reinterpret_cast<float *>(lds + m.vr);
    int *flags = reinterpret_cast<int *>(lds + m.flags);
    int *list = reinterpret_cast<int *>(lds + m.lists) + wave * 2 * kLargeWaves;
    const int tree0 = (int)blockIdx.x * m.T, tree = tree0 + wave;
    const bool on = wave < m.T && tree < P.B && tree_active(P, tree);          // wave-uniform

    // every tree of the workgroup switched off (smz_set_active) or beyond the batch: all four wavefronts leave here, before the
    // rounds' barriers
    if (lane == 0) flags[wave] = on ? 1 : 0;
    __syncthreads();
    if ((flags[0] | flags[1] | flags[2] | flags[3]) == 0) return;

    const LaLds L = la_lds(A, (size_t)m.trees + (size_t)(wave < m.T ? wave : 0) * m.per_tree);
    LaRng<PHX> R = {};
    if (on) R.load(P, tree, L.mt);

    // ---- simulations: two workgroup barriers per round (+ those inside large_tile), reached by all four wavefronts ----------
    for (int s = 0; s < sims; s++) {
        LaLeaf lf = {0, -1, 0, 0};
        if (on) lf = la_select_tree(P, tree, L, R);
        if (lane == 0) recs[wave] = make_int4(lf.parent_id, lf.action, lf.branch, lf.leaf_id);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();                                                                                   // (1) leaf records
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // every wavefront lists the leaves per branch by itself (its own list in LDS): the same lists in all four
        const int4 r = recs[lane < kLargeWaves ? lane : 0];
        const bool dyn = lane < kLargeWaves && r.w >= 0 && r.z != 0, ady = lane < kLargeWaves && r.w >= 0 && r.z == 0;
        const unsigned long long m_dyn = __ballot(dyn), m_ady = __ballot(ady), below = (1ull << lane) - 1ull;
        if (dyn) list[__popcll(m_dyn & below)] = lane;
        if (ady) list[kLargeWaves + __popcll(m_ady & below)] = lane;
        lds_sync();
        const int n0 = __popcll(m_dyn), n1 = __popcll(m_ady);
#pragma unroll 1
        for (int b = 0; b < 2; b++) {
            const int count = b ? n1 : n0;                                   // (the same in all four wavefronts)
            if (count == 0) continue;
            const int *li = list + b * kLargeWaves;
            // inputs: the parent's hidden row and the action; outputs: the new node's row of the handle's hidden array, the
            // tree's policy work row, its (value, reward) slot
            smz_mlp::large_tile<kLargeWaves>(d, weights, tile, count, b != 0, lane, wave, xw,
                                             [&](int j, int k) {
                                                 const int sl = li[j];
                                                 return P.hidden[((size_t)(tree0 + sl) * P.N + recs[sl].x) * P.hs + k];
                                             },
                                             [&](int j) { return recs[li[j]].y; },
                                             [&](int j) {
                                                 const int sl = li[j];
                                                 return WideDst{P.hidden + ((size_t)(tree0 + sl) * P.N + recs[sl].w) * P.hs,
                                                                policy_work + (size_t)(tree0 + sl) * A, vr + 2 * sl, vr + 2 * sl + 1};
                                             });
        }
        // the wavefronts wrote panels of policy rows and hidden rows (global) and value / reward (LDS) of trees other wavefronts
        // own: workgroup-scope release / acquire around the barrier
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();                                                                                   // (2) results
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (on) {
            const float value = vr[2 * wave], reward = vr[2 * wave + 1];
            la_expand_backup_tree<false>(P, tree, L, R, reward, policy_work + (size_t)tree * A, value);
            la_sync();                                                       // what lane 0 stored to the tree, the next selection loads
        }
    }
    if (on) R.save(P, tree);
}

int search_mlp_large_launch(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *hidden0_dev,
                            const float *policy0_dev, int train, ActOut act, const double *pow_table_host, smz_stream stream) {
    if (!h || !desc || !weights_dev || !hidden0_dev || !policy0_dev) return fail(SMZ_ERR_INVALID, "smz_search_mlp_large: null argument%s");
    if (!h->large_actions)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_large: not a large-action handle (per-lane handles use smz_search_mlp / smz_search_mlp_wide)%s");
    if (h->P.n_cycle > 1) return refuse_multi_player("smz_search_mlp_large");
    {
        smz_mlp_desc t = *desc;
        bool same = smz_mlp_layout_large(&t) == SMZ_OK && t.total_floats == desc->total_floats && desc->OP == kWideOP;
        for (int m = 0; same && m < 2 * M_COUNT; m++) same = t.off[m] == desc->off[m];
        if (!same)
            return fail(SMZ_ERR_INVALID, "smz_search_mlp_large: descriptor does not describe a large-action mlp_model weight buffer (smz_mlp_layout_large)%s");
    }
    if (desc->A != h->P.A || desc->S != h->P.S)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_large: network dimensions differ from the handle's%s");
    if (const int rc = check_dirichlet_alpha(h, train)) return rc;
    DeviceGuard guard(h->cfg.device);
    Params P = h->P;
    // trees per workgroup: every CU has a workgroup before any workgroup takes a second tree, up to the most that fit
    // (large_search_lds).  A workgroup with one tree evaluates one tile per round, one with several usually both branches' tiles
    // one after the other, and waits for its slowest selection: at 256 trees one tree per workgroup searches 1.3-1.6 times as
    // fast as four, at 512 two beat both one and four (profiles/r15_large_single_launch_trees_per_wg_ab.txt).  The environment
    // variable SMZ_LARGE_SEARCH_T (1 .. 4) replaces the count (A/B runs and tests: a search does not depend on the geometry).
    int want = (P.B + kCus - 1) / kCus;
    if (const char *e = getenv("SMZ_LARGE_SEARCH_T")) {
        const int v = atoi(e);
        if (v >= 1) want = v;
    }
    const LargeSearchLds ml = large_search_lds(P.A, want);
    P.tpw = want;
    if (ml.T < 1) return fail(SMZ_ERR_TOO_LARGE, "smz_search_mlp_large: working set exceeds the 160 KB LDS of a CU%s");
    if (!h->d_la_policy) {                   // the policy work rows [B][A]: the handle's, freed with it
        if (const int rc = dev_alloc(h, &h->d_la_policy, (size_t)P.B * (size_t)P.A)) return rc;
    }
    if (act.action && use_pow_table(h, P, act.temperature, pow_table_host, stream) != SMZ_OK) return SMZ_ERR_HIP;
    // root: the step-wise kernels (k_root_init_la, and k_root_noise_la behind it when training)
    if (const int rc = smz_internal_la_root_init(h, hidden0_dev, policy0_dev, nullptr, train, stream)) return rc;
    if (P.sims > 0) {
        const int blocks = (P.B + ml.T - 1) / ml.T;
        const int rc = P.philox ? launch_with_lds<k_search_mlp_large<true>>(h, blocks, kLargeWaves * kWave, (size_t)ml.total, stream, P, *desc,
                                                                           weights_dev, h->d_la_policy)
                                : launch_with_lds<k_search_mlp_large<false>>(h, blocks, kLargeWaves * kWave, (size_t)ml.total, stream, P, *desc,
                                                                            weights_dev, h->d_la_policy);
        if (rc != SMZ_OK) return rc;
        if (const int rc2 = launch_check()) return rc2;
    }
    if (act.action) {
        if (const int rc = smz_internal_la_act(h, P, act.temperature, act.action, act.policy, act.child_visits, act.root_value, stream))
            return rc;
    }
    // (the name as rocprofv3 prints it; with num_simulations == 0 the rounds kernel is not launched at all)
    snprintf(h->last_kernel, sizeof(h->last_kernel), P.philox ? "k_search_mlp_large<true>" : "k_search_mlp_large<false>");
    return search_launched(h);
}

}  // namespace

extern "C" {

int smz_search_mlp_large(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *hidden0_dev,
                         const float *policy0_dev, int train, smz_stream stream) {
    return search_mlp_large_launch(h, desc, weights_dev, hidden0_dev, policy0_dev, train, kNoAct, nullptr, stream);
}

int smz_search_mlp_large_act(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *hidden0_dev,
                             const float *policy0_dev, int train, double temperature, const double *pow_table_host,
                             int32_t *action_dev, double *policy_dev, double *child_visits_dev, float *root_value_dev,
                             smz_stream stream) {
    if (const int rc = check_act_outputs("smz_search_mlp_large_act", action_dev, policy_dev, child_visits_dev)) return rc;
    return search_mlp_large_launch(h, desc, weights_dev, hidden0_dev, policy0_dev, train,
                                   ActOut{temperature, action_dev, policy_dev, child_visits_dev, root_value_dev}, pow_table_host, stream);
}

}  // extern "C"
