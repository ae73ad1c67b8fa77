// smz_large_actions.hip -- the step-wise tree kernels for 1 <= A <= SMZ_MAX_ACTIONS_LARGE actions (smz_create_large_actions).
//
// Execution shape: ONE wavefront per tree, one wavefront per workgroup (B workgroups).  The per-lane kernels of smz_kernels.hip
// keep a tree's A-wide arrays in registers, which stops at A = 32; here the lanes split the A-wide loops and the arrays live
// in this wave's LDS.  What numpy defines as sequential stays sequential (the float64 cumsum of RandomState.choice, the
// Dirichlet gammas and their sum, the backup's value chain); every lane then computes the same scalar values, so control flow
// stays uniform over the wave.  Everything else -- normalisation, the searchsorted of a round's draws, the pUCT scores of a
// level, the one-hot network input -- runs a child or a draw per lane.  The arithmetic is smz_device.hpp's (puct_score,
// legacy_gamma, np_sum, the glibc math), called, not restated: the trees are bit-identical to the per-lane kernels'.
//
// Tree layout, node ids and hidden rows are those of smz_device.hpp.  One difference: a path record names its child as
// block << kLaSlotBits | slot (a root slot may exceed 255); smz_debug_dump_tree decodes it by the handle's kind.
//
// Random words: the wave keeps its tree's 624 MT19937 words in LDS for the launch and twists them 64 at a time in place (the
// words i .. i + 63 read words i + 397 mod 624 of the same pass only at least 227 words back, so a 64-word chunk is
// parallel-safe), then writes them back with the (ready << 16 | idx) position of the per-lane kernels.  Philox handles
// compute each word where it is needed (philox_word).  Both consume exactly the per-lane kernels' words, in their order.
//
// The device code -- LaLds, LaRng, the choice / cdf / argmax helpers and the bodies of selection and expansion + backup
// (la_select_tree, la_expand_backup_tree) -- lives in smz_large_actions_device.hpp, shared with the whole-search kernel
// k_search_mlp_large (smz_mlp_large_search.hip); k_select_la and k_expand_backup_la load the generator, call and save.
//
// Build: same flags as smz_kernels.hip (-ffp-contract=off: no fused multiply-add).
#include "smz_common.hpp"
#include "smz_handle.hpp"
#include "smz_large_actions_device.hpp"      // LaLds, LaRng, la_choice, ..., la_select_tree, la_expand_backup_tree

namespace {

// ---------------------------------------------------------------------------------------------------------------
// root (monte_carlo_tree_search.py:179-225): root_init_tree
// ---------------------------------------------------------------------------------------------------------------
template <bool PHX>
__global__ void __launch_bounds__(kWave) k_root_init_la(Params P, const float *hidden, const float *policy,
                                                        const double *noise_override, int train) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B || !tree_active(P, tree)) return;
    const int A = P.A;
    const LaLds L = la_lds(A);
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
    uint32_t *rb = tree_base(P, tree);
    la_normalise_policy(policy + (size_t)tree * A, A, L);
    int32_t *vi = (int32_t *)rb;
    float *fs = (float *)rb;
    for (int a = lane; a < A; a += kWave) {
        vi[2 * a] = 0;
        fs[2 * a + 1] = 0.f;
        fs[2 * A + a] = 0.f;
        fs[3 * A + a] = L.f[a];
        vi[4 * A + a] = 0;
    }
    la_choice(R, A, A, L);          // sorted result is 0..A-1; only the draws matter (mcts:208)
    double *rp = (double *)(rb + P.rp_off);
    if (!(train && P.sims > 0))
        for (int a = lane; a < A; a += kWave) rp[a] = (double)L.f[a];
    R.save(P, tree);
    if (lane == 0) {
        TreeHdr h;
        h.n_exp = 0;
        h.path_len = 0;
        h.mn = __builtin_inff();
        h.mx = -__builtin_inff();
        h.root_visit = 0;
        h.root_value_sum = 0.f;
        h.pad0 = h.pad1 = 0;
        P.hdr[tree] = h;
    }
    if (P.S > 0 && hidden) la_copy_row(hidden + (size_t)tree * P.S, P.hidden + (size_t)tree * P.N * P.hs, P.S);
}

// ... and its Dirichlet noise (mcts:216-225), a launch of its own behind it (train, num_simulations > 0): the glibc log / pow of
// the gammas beside the choice rounds would not fit the scalar registers
template <bool ONE, bool PHX>
__global__ void __launch_bounds__(kWave) k_root_noise_la(Params P, const double *noise_override) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B || !tree_active(P, tree)) return;
    const int A = P.A;
    const LaLds L = la_lds(A);
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
    uint32_t *rb = tree_base(P, tree);
    // A legacy gammas in stream order, summed in the same order (one chain: la_cumsum's last entry)
    la_dirichlet_gammas<ONE>(R, P.alpha, A, L.d0);
    la_cumsum(L.d0, L.d1, A);
    const double inv = 1.0 / L.d1[A - 1];
    const double *ov = noise_override ? noise_override + (size_t)tree * A : nullptr;
    double *rp = (double *)(rb + P.rp_off);
    for (int a = lane; a < A; a += kWave) {
        const double n = ov ? ov[a] : L.d0[a] * inv;
        const float scaled = __uint_as_float(rb[3 * A + a]) * P.keep32;
        rp[a] = (double)scaled + n * P.frac;
    }
    R.save(P, tree);
}

// ---------------------------------------------------------------------------------------------------------------
// selection (monte_carlo_tree_search.py:228-267): la_select_tree
// ---------------------------------------------------------------------------------------------------------------
template <bool PHX>
__global__ void __launch_bounds__(kWave) k_select_la(Params P, float *parent_hidden, int32_t *last_action, uint8_t *branch,
                                                     float *mlp_input) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B) return;
    if (!tree_active(P, tree)) {
        if (P.ids_out && lane == 0) { P.ids_out[2 * (size_t)tree] = -1; P.ids_out[2 * (size_t)tree + 1] = -1; }
        return;
    }
    const int A = P.A;
    const LaLds L = la_lds(A);
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
    const LaLeaf lf = la_select_tree(P, tree, L, R);
    R.save(P, tree);
    if (lane == 0) {
        if (last_action) last_action[tree] = lf.action;
        if (branch) branch[tree] = (uint8_t)lf.branch;
        if (P.ids_out) { P.ids_out[2 * (size_t)tree] = lf.leaf_id; P.ids_out[2 * (size_t)tree + 1] = lf.parent_id; }
    }
    if (P.S > 0 && (parent_hidden || mlp_input)) {
        const int S = P.S, W = S + A;
        const float *src = P.hidden + ((size_t)tree * P.N + lf.parent_id) * P.hs;
        for (int i = lane; i < (mlp_input ? W : S); i += kWave) {
            const float v = i < S ? src[i] : ((i - S) == lf.action ? 1.0f : 0.0f);
            if (mlp_input) mlp_input[(size_t)tree * W + i] = v;
            if (parent_hidden && i < S) parent_hidden[(size_t)tree * S + i] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// expansion + backup (monte_carlo_tree_search.py:282-308): la_expand_backup_tree; MP = the multi-player sign rule
// ---------------------------------------------------------------------------------------------------------------
template <bool MP, bool PHX>
__global__ void __launch_bounds__(kWave) k_expand_backup_la(Params P, const float *hidden, const float *reward,
                                                            const float *policy, const float *value) {
    const int tree = blockIdx.x;
    if (tree >= P.B || !tree_active(P, tree)) return;
    const int A = P.A;
    const LaLds L = la_lds(A);
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
    const int leaf = la_expand_backup_tree<MP>(P, tree, L, R, reward ? reward[tree] : 0.0f, policy + (size_t)tree * A, value[tree]);
    R.save(P, tree);
    if (P.S > 0 && hidden) la_copy_row(hidden + (size_t)tree * P.S, P.hidden + ((size_t)tree * P.N + leaf) * P.hs, P.S);
}

// ---------------------------------------------------------------------------------------------------------------
// post-search policy / action (game.py:179-232): act_tree
// ---------------------------------------------------------------------------------------------------------------
template <bool PHX>
__global__ void __launch_bounds__(kWave) k_act_la(Params P, double temperature, int32_t *action_out, double *policy_out,
                                                  double *child_visits_out, float *root_value_out) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B || !tree_active(P, tree)) return;
    const int A = P.A;
    const LaLds L = la_lds(A);
    const uint32_t *rb = tree_base(P, tree);
    const double *rp = (const double *)(rb + P.rp_off);
    double *vis = L.d0, *pol = L.d1, *cdf = L.d2;
    for (int a = lane; a < A; a += kWave) vis[a] = (double)(int32_t)rb[2 * a];
    la_sync();
    const double vsum = la_sum<double>(vis, A);
    const bool from_visits = !(vsum <= 1.0);
    bool eq = true;
    const bool table = temperature >= 0.3 && from_visits && P.pow_table;
    for (int a = lane; a < A; a += kWave) pol[a] = table ? P.pow_table[(int32_t)rb[2 * a]] : (from_visits ? vis[a] : rp[a]);
    if (temperature >= 0.3 && !table) {                 // (numpy's ** = libm's pow)
        const double e = 1.0 / temperature;
        for (int a = lane; a < A; a += kWave) pol[a] = smz_glibc_pow(pol[a], e);
    }
    la_sync();
    const double ps = la_sum<double>(pol, A);
    la_sync();
    for (int a = lane; a < A; a += kWave) pol[a] = pol[a] / ps;
    la_sync();
    for (int a = lane; a < A; a += kWave) eq = eq && (pol[a] == pol[0]);
    const bool all_equal = __ballot(!eq) == 0ull;
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
    int pick = 0;
    if (temperature > 0.1 || all_equal) {
        pick = la_sample_cdf(pol, cdf, A, R.random_sample());
    } else {
        double best = 0.0;
        int bj = -1;
        for (int a = lane; a < A; a += kWave) if (bj < 0 || pol[a] > best) { best = pol[a]; bj = a; }
        la_argmax_first(best, bj);
        pick = bj;
    }
    R.save(P, tree);
    if (action_out && lane == 0) action_out[tree] = pick;
    if (policy_out) for (int a = lane; a < A; a += kWave) policy_out[(size_t)tree * A + a] = pol[a];
    if (child_visits_out) {
        if (vsum >= 3.0) {
            for (int a = lane; a < A; a += kWave) child_visits_out[(size_t)tree * A + a] = vis[a] / vsum;
        } else {
            for (int a = lane; a < A; a += kWave) cdf[a] = rp[a];
            la_sync();
            const double s = la_sum<double>(cdf, A);
            for (int a = lane; a < A; a += kWave) child_visits_out[(size_t)tree * A + a] = rp[a] / s;
        }
    }
    if (root_value_out && lane == 0) {
        const TreeHdr h = P.hdr[tree];
        root_value_out[tree] = h.root_visit ? h.root_value_sum / (float)h.root_visit : 0.0f;
    }
}

inline dim3 la_grid(const Params &P) { return dim3((unsigned)P.B); }

}  // namespace

// ---- entry points of smz_kernels.hip for large-action handles (smz_handle::large_actions) --------------------------------
#define SMZ_LA_LAUNCH(KERNEL, P, ...)                                                                                         \
    do {                                                                                                                     \
        if ((P).philox) hipLaunchKernelGGL((KERNEL<__VA_ARGS__ true>), la_grid(P), dim3(kWave), la_lds_bytes((P).A), (hipStream_t)stream, \
                                          (P), SMZ_LA_ARGS);                                                                  \
        else hipLaunchKernelGGL((KERNEL<__VA_ARGS__ false>), la_grid(P), dim3(kWave), la_lds_bytes((P).A), (hipStream_t)stream, \
                                (P), SMZ_LA_ARGS);                                                                            \
    } while (0)

int smz_internal_la_root_init(smz_handle *h, const float *hidden_dev, const float *policy_dev, const double *noise_override_dev,
                              int train, smz_stream stream) {
#define SMZ_LA_ARGS hidden_dev, policy_dev, noise_override_dev, train
    SMZ_LA_LAUNCH(k_root_init_la, h->P, );
#undef SMZ_LA_ARGS
    if (train && h->P.sims > 0) {
#define SMZ_LA_ARGS noise_override_dev
        if (h->P.alpha == 1.0) SMZ_LA_LAUNCH(k_root_noise_la, h->P, true,);      // Dirichlet(1): one uniform per gamma
        else SMZ_LA_LAUNCH(k_root_noise_la, h->P, false,);
#undef SMZ_LA_ARGS
    }
    return launch_check();
}

int smz_internal_la_select(smz_handle *h, float *parent_hidden_dev, int32_t *last_action_dev, uint8_t *branch_dev,
                           float *mlp_input_dev, smz_stream stream) {
#define SMZ_LA_ARGS parent_hidden_dev, last_action_dev, branch_dev, mlp_input_dev
    SMZ_LA_LAUNCH(k_select_la, h->P, );
#undef SMZ_LA_ARGS
    return launch_check();
}

int smz_internal_la_expand_backup(smz_handle *h, const float *hidden_dev, const float *reward_dev, const float *policy_dev,
                                  const float *value_dev, smz_stream stream) {
#define SMZ_LA_ARGS hidden_dev, reward_dev, policy_dev, value_dev
    if (h->P.n_cycle > 1) SMZ_LA_LAUNCH(k_expand_backup_la, h->P, true,);     // multi-player backup (smz_set_players)
    else SMZ_LA_LAUNCH(k_expand_backup_la, h->P, false,);
#undef SMZ_LA_ARGS
    return launch_check();
}

int smz_internal_la_act(smz_handle *h, const Params &P, double temperature, int32_t *action_dev, double *policy_dev,
                        double *child_visits_dev, float *root_value_dev, smz_stream stream) {
#define SMZ_LA_ARGS temperature, action_dev, policy_dev, child_visits_dev, root_value_dev
    SMZ_LA_LAUNCH(k_act_la, P, );
#undef SMZ_LA_ARGS
    return launch_check();
}
#undef SMZ_LA_LAUNCH
