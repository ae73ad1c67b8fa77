// smz_kernels.hip -- the step-wise kernels, the handle and most of the C ABI of libsmz.so (see include/smz.h for the contract).
//
// Execution shape: one search tree per lane, one 64-lane wavefront per workgroup, ceil(B/64) workgroups.  The
// per-tree control flow (descent depth, rejection loops of the numpy samplers) is data dependent, so trees are
// kept on separate lanes and diverge freely; the only wave-cooperative parts are the row moves of hidden states
// (parent -> network input, network output -> leaf), where the lanes of a wave walk its 64 trees together so that
// each row is read and written as one contiguous segment instead of 64 strided dwords.
//
// The library's other translation units: smz_fused.hip (smz_expand_backup_select), smz_search.hip, smz_search_wide.hip and
// smz_search_lds.hip (the single-launch mlp_model search, split by instantiation: the template instantiations are most of
// the compile time, and the units build in parallel), the add-on searches and the head kernels.  Shared code lives in
// smz_common.hpp, smz_stepwise.hpp, smz_search_mlp.hpp and smz_handle.hpp.
#include "smz_common.hpp"
#include "smz_stepwise.hpp"
#include "smz_handle.hpp"

namespace {

// numpy `seed(int)`: init_genrand (numpy/random/src/mt19937/mt19937.c mt19937_seed); pos = 624.
__global__ void __launch_bounds__(kWave) k_seed(Params P, const uint64_t *seeds) {
    const int tree = blockIdx.x * kWave + threadIdx.x;
    if (tree >= P.B) return;
    if (P.philox) {          // counter-based stream: the seed is the key, nothing else to initialise
        const_cast<uint32_t *>(P.rng_key)[2 * tree] = (uint32_t)(seeds[tree] & 0xffffffffull);
        const_cast<uint32_t *>(P.rng_key)[2 * tree + 1] = (uint32_t)(seeds[tree] >> 32);
        P.rng_block[tree] = 0u;
        P.rng_pos[tree] = 0;
        return;
    }
    uint32_t s = (uint32_t)(seeds[tree] & 0xffffffffull);
    uint32_t *mt = P.mt + (size_t)tree * kMtN;
    for (int i = 0; i < kMtN; i++) {
        mt[i] = s;
        s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)i + 1u;
    }
    P.rng_pos[tree] = 0;  // idx 0, nothing pre-twisted: the first draw twists word 0 (== numpy pos 624)
}

__global__ void __launch_bounds__(kWave) k_root_stats(Params P, int32_t *visits, double *priors, float *root_value,
                                                      float *child_reward) {
    const int tree = blockIdx.x * kWave + threadIdx.x;
    if (tree >= P.B) return;
    const uint32_t *rb = tree_base(P, tree);
    const double *rp = (const double *)(rb + P.rp_off);
    for (int a = 0; a < P.A; a++) {
        if (visits) visits[(size_t)tree * P.A + a] = (int32_t)rb[2 * a];
        if (priors) priors[(size_t)tree * P.A + a] = rp[a];
        if (child_reward) child_reward[(size_t)tree * P.A + a] = __uint_as_float(rb[2 * P.A + a]);
    }
    if (root_value) {
        const TreeHdr h = P.hdr[tree];
        root_value[tree] = h.root_visit ? h.root_value_sum / (float)h.root_visit : 0.0f;
    }
}

template <int MAXA>
__global__ void __launch_bounds__(kWave) k_act(Params P, double temperature, int32_t *action, double *policy,
                                               double *child_visits, float *root_value) {
    const int tree = blockIdx.x * kWave + threadIdx.x;
    if (tree >= P.B || !tree_active(P, tree)) return;
    Rng rng;
    rng.bind(P, tree, true);
    rng.load(P.mt + (size_t)tree * kMtN, P.rng_pos[tree], nullptr, 0);
    act_tree<MAXA>(P, tree, rng, temperature, action, policy, child_visits, root_value);
    P.rng_pos[tree] = rng.pack();
    rng.save(P, tree);
}

// ---- head epilogues: `lpr` lanes cooperate on one row (coalesced loads, shuffle reductions) ------------------------
__device__ inline float grp_max(float v, int lpr) {
    for (int off = lpr >> 1; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ inline float grp_min(float v, int lpr) {
    for (int off = lpr >> 1; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}
__device__ inline float grp_sum(float v, int lpr) {
    for (int off = lpr >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// inverse_transform_with_support of one row by a lane group (muzero_model.py:575-591); every lane gets the result
__device__ inline float support_decode_group(const float *row, int S, int li, int lpr) {
    float m = -__builtin_inff();
    for (int i = li; i < S; i += lpr) m = fmaxf(m, row[i]);
    m = grp_max(m, lpr);
    float den = 0.f, num = 0.f;
    const int half = S / 2;
    for (int i = li; i < S; i += lpr) {
        const float e = expf(row[i] - m);
        den += e;
        num += (float)(i - half) * e;
    }
    den = grp_sum(den, lpr);
    num = grp_sum(num, lpr);
    const float y = num / den;
    const float sg = (y > 0.f) ? 1.f : ((y < 0.f) ? -1.f : 0.f);
    const float r = (sqrtf(1.f + 4.f * 0.001f * (fabsf(y) + 1.f + 0.001f)) - 1.f) / (2.f * 0.001f);
    return sg * (r * r - 1.f);
}

__device__ inline void softmax_group(const float *row, int A, float *out, int li, int lpr) {
    float m = -__builtin_inff();
    for (int i = li; i < A; i += lpr) m = fmaxf(m, row[i]);
    m = grp_max(m, lpr);
    float den = 0.f;
    for (int i = li; i < A; i += lpr) den += expf(row[i] - m);
    den = grp_sum(den, lpr);
    for (int i = li; i < A; i += lpr) out[i] = expf(row[i] - m) / den;
}

__global__ void __launch_bounds__(256) k_support_decode(const float *logits, int S, float *out, int B, int lpr) {
    const int gid = (blockIdx.x * blockDim.x + threadIdx.x) / lpr, li = threadIdx.x % lpr;
    const int row = gid < B ? gid : B - 1;     // surplus groups recompute the last row (keeps shuffles convergent)
    const float v = support_decode_group(logits + (size_t)row * S, S, li, lpr);
    if (gid < B && li == 0) out[row] = v;
}

__global__ void __launch_bounds__(256) k_policy_softmax(const float *logits, int A, float *out, int B, int lpr) {
    const int gid = (blockIdx.x * blockDim.x + threadIdx.x) / lpr, li = threadIdx.x % lpr;
    if (gid < B) softmax_group(logits + (size_t)gid * A, A, out + (size_t)gid * A, li, lpr);
    else { float dummy[1]; softmax_group(logits + (size_t)(B - 1) * A, 0, dummy, li, lpr); }
}

__global__ void __launch_bounds__(256) k_dynamics_epilogue(const float *state_dyn, const float *state_after,
                                                           const float *reward_logits, int ld, const uint8_t *branch,
                                                           int S, float *hidden_out, float *reward_out, int B, int lpr) {
    const int gid = (blockIdx.x * blockDim.x + threadIdx.x) / lpr, li = threadIdx.x % lpr;
    const int row = gid < B ? gid : B - 1;
    const bool live = gid < B;
    const bool dyn = branch[row] != 0;
    const float *x = (dyn ? state_dyn : state_after) + (size_t)row * ld;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int i = li; i < S; i += lpr) { const float v = x[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    mn = grp_min(mn, lpr);
    mx = grp_max(mx, lpr);
    float sc = mx - mn;
    if (sc < 1e-5f) sc += 1e-5f;  // neural_network_mlp_model.py:353
    if (live) for (int i = li; i < S; i += lpr) hidden_out[(size_t)row * S + i] = (x[i] - mn) / sc;
    if (reward_out) {
        float r = 0.f;
        if (reward_logits) r = support_decode_group(reward_logits + (size_t)row * ld, S, li, lpr);
        if (live && li == 0) reward_out[row] = dyn ? r : 0.f;
    }
}

__global__ void __launch_bounds__(256) k_prediction_epilogue(const float *pol_pred, const float *val_pred,
                                                             const float *pol_after, const float *val_after,
                                                             int ld, const uint8_t *branch, int A, int S,
                                                             float *policy_out, float *value_out, int B, int lpr) {
    const int gid = (blockIdx.x * blockDim.x + threadIdx.x) / lpr, li = threadIdx.x % lpr;
    const int row = gid < B ? gid : B - 1;
    const bool live = gid < B;
    const bool dyn = branch[row] != 0;
    const float *pl = (dyn ? pol_pred : pol_after) + (size_t)row * ld;
    float m = -__builtin_inff();
    for (int i = li; i < A; i += lpr) m = fmaxf(m, pl[i]);
    m = grp_max(m, lpr);
    float den = 0.f;
    for (int i = li; i < A; i += lpr) den += expf(pl[i] - m);
    den = grp_sum(den, lpr);
    if (live) for (int i = li; i < A; i += lpr) policy_out[(size_t)row * A + i] = expf(pl[i] - m) / den;
    const float v = support_decode_group((dyn ? val_pred : val_after) + (size_t)row * ld, S, li, lpr);
    if (live && li == 0) value_out[row] = v;
}

// ---- synthetic env + trajectory record ---------------------------------------------------------------------------
// one thread per env; traj != nullptr: also appends the step's record -- one launch less per env step
__global__ void __launch_bounds__(256) k_cartpole_step_env(EnvStep E, const int32_t *action, int B, const double *policy,
                                                           const double *child_visits, const float *root_value) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B) return;
    cartpole_env_step(E, e, B, action, policy, child_visits, root_value);
}

// N(0,1) float32 observations of a stand-in env (Box-Muller on two counter-based uniforms), env-major [B][obs_dim]
__global__ void __launch_bounds__(256) k_synthetic_obs(float *obs, int B, int obs_dim, uint64_t seed, long long first_env,
                                                       long long t) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * obs_dim) return;
    const uint64_t e = (uint64_t)(first_env + (long long)(i / obs_dim)), k = (uint64_t)(i % obs_dim);
    const double u1 = 1.0 - smz_unit(seed, e, (uint64_t)t, 2 * k), u2 = smz_unit(seed, e, (uint64_t)t, 2 * k + 1);
    obs[i] = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2));
}

// record layout per (step, env):
//   [obs(obs_dim) | reward | terminated | policy(A) | action one-hot(A) | root_value | child_visits(A)]
// One thread per float64 of the step's [B][F] slab: writes are contiguous across the whole slab and the observation
// reads are contiguous per row, whatever obs_dim is (4 for CartPole, 28812 for a 98x98x3 frame).
__global__ void __launch_bounds__(256) k_traj_pack(double *traj, int T, int t, int obs_dim, int A, const float *obs,
                                                   const float *reward, const uint8_t *terminated, const int32_t *action,
                                                   const double *policy, const double *child_visits,
                                                   const float *root_value, int B) {
    const int F = obs_dim + 3 * A + 3;
    const size_t total = (size_t)B * F;
    double *slab = traj + (size_t)t * total;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(i / F), k = (int)(i % F);
        double v;
        if (k < obs_dim) v = (double)obs[(size_t)e * obs_dim + k];
        else if (k == obs_dim) v = reward ? (double)reward[e] : 0.0;
        else if (k == obs_dim + 1) v = terminated ? (double)terminated[e] : 0.0;     // the flag itself: 0 / 1 / 2 / 3
        else {
            const int j = k - obs_dim - 2;
            if (j < A) v = policy[(size_t)e * A + j];
            else if (j < 2 * A) v = (j - A == action[e]) ? 1.0 : 0.0;
            else if (j == 2 * A) v = (double)root_value[e];
            else v = child_visits[(size_t)e * A + (j - 2 * A - 1)];
        }
        slab[i] = v;
    }
}

// Game length of every env of a chunk: steps up to and including the first terminated one (chunk_to_games'/play_game's
// cut, self_play.py:79-94), or T.
__global__ void __launch_bounds__(256) k_traj_lengths(const double *traj, int T, int obs_dim, int A, int B, int ignore_term,
                                                      int32_t *length) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B) return;
    const int F = obs_dim + 3 * A + 3;
    int n = T;
    if (!ignore_term)
        for (int t = 0; t < T; t++)
            if (traj[((size_t)t * B + e) * F + obs_dim + 1] != 0.0) { n = t + 1; break; }
    length[e] = n;
}

// Several games per env and chunk (on_end = "reset"; chunk_to_games(after_end = "new_game")): game_end[t][e] = one past the
// last row of the game that row t of env e belongs to -- the row of its end flag (1 terminated / 2 step limit) + 1, or T
// for the unfinished game at the end of the chunk; -1 for a row without a step (flag 3).  new_game == 0: rows behind the
// first finished game belong to no game (the cut of k_traj_lengths).  length[e] = end of the env's first game.
__global__ void __launch_bounds__(256) k_traj_game_ends(const double *traj, int T, int obs_dim, int A, int B, int ignore_term,
                                                        int new_game, int32_t *length, int32_t *game_end) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B) return;
    const int F = obs_dim + 3 * A + 3;
    int end = T, first = T;
    for (int t = T - 1; t >= 0; t--) {
        const int flag = ignore_term ? 0 : (int)traj[((size_t)t * B + e) * F + obs_dim + 1];
        if (flag == 3) { end = t; game_end[(size_t)t * B + e] = -1; continue; }
        if (flag != 0) end = t + 1;
        game_end[(size_t)t * B + e] = end;
        first = end;
    }
    if (!new_game)
        for (int t = first; t < T; t++) game_end[(size_t)t * B + e] = -1;
    if (length) length[e] = first;
}

// n-step value target of every stored position (the value entry of Game.make_target and the target inside
// Game.make_priority, game.py:291-337), with the reference's scalar types: root values are numpy float32, rewards and
// discount powers Python floats, so under NEP 50 a bootstrapped chain (position + td_steps inside the game) runs in
// float32 -- f32(root_value) * f32(discount^td), then one f32 add per reward of the f64 product reward * discount^i
// rounded to f32 -- and a chain past the end of the game starts from a Python 0 and stays float64.
// abs_td = |float64(root_value[t]) - target| (make_priority before ** priority_scale).  Positions t >= length are 0.
__global__ void __launch_bounds__(256) k_traj_targets(const double *traj, int T, int obs_dim, int A, int B, int td,
                                                      const double *disc_pow, const int32_t *length, double *target,
                                                      double *abs_td, const int32_t *game_end = nullptr) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)T * B) return;
    const int t = (int)(i / B), e = (int)(i % B);
    // (a game that starts inside the chunk: positions, bootstrap index and end are all chunk rows, so the arithmetic of a
    // game-relative index is unchanged)
    const int F = obs_dim + 3 * A + 3, n = game_end ? game_end[i] : length[e];
    const size_t rv_off = obs_dim + 2 + 2 * A;
    double out = 0.0, err = 0.0;
    if (t < n) {
        const int b = t + td;
        if (b < n) {
            float v = (float)traj[((size_t)b * B + e) * F + rv_off] * (float)disc_pow[td];
            for (int k = 0; k < td; k++) v = v + (float)(traj[((size_t)(t + k) * B + e) * F + obs_dim] * disc_pow[k]);
            out = (double)v;
        } else {
            double v = 0.0;
            for (int k = 0; t + k < n; k++) v += traj[((size_t)(t + k) * B + e) * F + obs_dim] * disc_pow[k];
            out = v;
        }
        err = fabs(traj[i * F + rv_off] - out);
    }
    target[i] = out;
    if (abs_td) abs_td[i] = err;
}

// div_by_count against the IEEE division, element-wise (inspection: tests pin the table-based quotients)
__global__ void __launch_bounds__(256) k_debug_div_by_count(const double *x, const int32_t *n, int count, int N, double *out) {
    for (int i = threadIdx.x; i < N; i += blockDim.x) smz_dyn_lds[i] = i > 0 ? 1.0 / (double)i : 0.0;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x)
        out[i] = div_by_count(x[i], n[i], smz_dyn_lds);
}

// glibc's log / pow as the device restates them (smz_glibc_math.hpp), element-wise (inspection: tests compare with the host's libm)
__global__ void __launch_bounds__(256) k_debug_glibc_log_pow(const double *x, const double *y, int count, double *out_log,
                                                             double *out_pow) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        if (out_log) out_log[i] = smz_glibc_log(x[i]);
        if (out_pow) out_pow[i] = smz_glibc_pow(x[i], y[i]);
    }
}

}  // namespace

thread_local char smz_g_err[512] = "";

namespace {
int create_handle(const smz_config *cfg, smz_handle **out, bool large_actions);
}

extern "C" {

const char *smz_last_error(void) { return g_err; }
int smz_abi_version(void) { return SMZ_ABI_VERSION; }
int smz_build_features(void) { return 0; }
int smz_node_capacity(const smz_handle *h) { return h ? h->N : SMZ_ERR_INVALID; }
int smz_last_kernel(const smz_handle *h, char *buf, int cap) {
    if (!h || !buf || cap < 1) return fail(SMZ_ERR_INVALID, "smz_last_kernel: bad argument%s");
    snprintf(buf, (size_t)cap, "%s", h->last_kernel);
    return (int)strlen(h->last_kernel);
}

int smz_create(const smz_config *cfg, smz_handle **out) { return create_handle(cfg, out, false); }
int smz_create_large_actions(const smz_config *cfg, smz_handle **out) { return create_handle(cfg, out, true); }
}  // extern "C"

namespace {
int create_handle(const smz_config *cfg, smz_handle **out, bool large_actions) {
    if (!cfg || !out) return fail(SMZ_ERR_INVALID, "smz_create: null argument%s");
    *out = nullptr;
    // hyper-parameter checks of monte_carlo_tree_search.py:148-173
    if (cfg->pb_c_base < 1) return fail(SMZ_ERR_INVALID, "pb_c_base must be an int >= 1%s");
    if (!(cfg->pb_c_init >= 0)) return fail(SMZ_ERR_INVALID, "pb_c_init must be a float >= 0%s");
    if (!(cfg->discount >= 0)) return fail(SMZ_ERR_INVALID, "discount must be >= 0%s");
    if (!(cfg->root_dirichlet_alpha >= 0 && cfg->root_dirichlet_alpha <= 1))
        return fail(SMZ_ERR_INVALID, "root_dirichlet_alpha must be in [0, 1]%s");
    if (!(cfg->root_exploration_fraction >= 0 && cfg->root_exploration_fraction <= 1))
        return fail(SMZ_ERR_INVALID, "root_exploration_fraction must be in [0, 1]%s");
    if (cfg->max_action_sample < 1) return fail(SMZ_ERR_INVALID, "maxium_action_sample must be an int >= 1%s");
    if (cfg->num_simulations < 0) return fail(SMZ_ERR_INVALID, "num_simulations must be an int >= 0%s");
    if (cfg->num_trees < 1) return fail(SMZ_ERR_INVALID, "num_trees must be >= 1%s");
    if (!large_actions && (cfg->num_actions < 1 || cfg->num_actions > SMZ_MAX_ACTIONS))
        return fail(SMZ_ERR_INVALID, "num_actions must be in [1, SMZ_MAX_ACTIONS]%s");
    if (large_actions && (cfg->num_actions < 1 || cfg->num_actions > SMZ_MAX_ACTIONS_LARGE))
        return fail(SMZ_ERR_INVALID, "num_actions must be in [1, SMZ_MAX_ACTIONS_LARGE] (smz_create_large_actions)%s");
    if (cfg->hidden_size < 0) return fail(SMZ_ERR_INVALID, "hidden_size must be >= 0%s");
    if (cfg->num_simulations > 32000) return fail(SMZ_ERR_INVALID, "num_simulations above 32000 is not supported%s");
    if (cfg->rng_mode != SMZ_RNG_MT19937_NUMPY && cfg->rng_mode != SMZ_RNG_PHILOX)
        return fail(SMZ_ERR_INVALID, "rng_mode must be SMZ_RNG_MT19937_NUMPY or SMZ_RNG_PHILOX%s");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(SMZ_ERR_INVALID, "device ordinal out of range%s");
    DeviceGuard guard(cfg->device);

    smz_handle *h = new (std::nothrow) smz_handle();
    if (!h) return fail(SMZ_ERR_NOMEM, "host allocation failed%s");
    h->cfg = *cfg;
    const int B = cfg->num_trees, A = cfg->num_actions, S = cfg->hidden_size, sims = cfg->num_simulations;
    h->K = cfg->max_action_sample < A ? cfg->max_action_sample : A;
    h->N = 1 + A + sims * h->K;
    h->Ppath = sims + 2;
    h->maxa = A <= 2 ? 2 : A <= 4 ? 4 : A <= 8 ? 8 : A <= 16 ? 16 : 32;
    h->root_ready = h->selected = false;
    h->pow_valid = false;
    h->d_player_neg = nullptr;
    h->large_actions = large_actions;
    h->d_la_policy = nullptr;
    h->pow_T = 0.0;
    h->stats_on = false;

    Params &P = h->P;
    memset(&P, 0, sizeof(P));
    P.B = B; P.A = A; P.K = h->K; P.S = S; P.N = h->N; P.P = h->Ppath; P.sims = sims;
    P.dbg = getenv("SMZ_DEBUG_SKIP") ? atoi(getenv("SMZ_DEBUG_SKIP")) : 0;
    {   // trees per wavefront: spread small batches over the whole chip (>= 1 wave per SIMD before packing lanes)
        int tpw = kWave;
        while (tpw > 1 && (B + tpw - 1) / tpw < 1024) tpw >>= 1;
        if (const char *e = getenv("SMZ_TREES_PER_WAVE")) {
            const int v = atoi(e);
            if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) tpw = v;
        }
        P.tpw = tpw;
        // the staged words live in a 16.6 KB LDS tile; SMZ_LDS_STAGE=0 twists ahead only and draws from L1 (measured
        // 7 % slower at 1 M trees: the large-batch regime is bound by cache-line transactions, not by occupancy)
        P.lds_stage = 1;
        if (const char *e = getenv("SMZ_LDS_STAGE")) P.lds_stage = atoi(e) ? 1 : 0;
    }
    P.disc32 = (float)cfg->discount;
    P.keep32 = (float)(1.0 - cfg->root_exploration_fraction);
    P.frac = cfg->root_exploration_fraction;
    P.alpha = cfg->root_dirichlet_alpha;
    const size_t BN = (size_t)B * h->N;
    // child-block geometry (16-word = 64-byte granules so that a block never straddles more lines than it must)
    P.rp_off = (5 * A + 1) & ~1;
    P.rb_words = ((P.rp_off + 2 * A) + 15) & ~15;
    P.eb_words = ((6 * h->K) + 15) & ~15;
    P.tree_words = (int64_t)P.rb_words + (int64_t)sims * P.eb_words;
    int rc = SMZ_OK;
    auto A_ = [&](int r) { if (rc == SMZ_OK) rc = r; };
    A_(dev_alloc(h, &P.nodes, (size_t)B * (size_t)P.tree_words));
    P.hs = (S + 15) & ~15;        // hidden rows start on 64-byte lines (S = 31 -> 128-byte rows: two whole lines)
    A_(dev_alloc(h, &P.hidden, BN * (size_t)P.hs));
    A_(dev_alloc(h, &P.hdr, (size_t)B));
    A_(dev_alloc(h, &P.path, (size_t)B * h->Ppath));
    A_(dev_alloc(h, &P.mt, (size_t)B * kMtN));
    A_(dev_alloc(h, &P.rng_pos, (size_t)B));
    A_(dev_alloc(h, &h->d_seeds, (size_t)B));
    A_(dev_alloc(h, &h->d_pbc, (size_t)sims + 2));
    A_(dev_alloc(h, &h->d_pow, (size_t)sims + 1));
    A_(dev_alloc(h, &h->d_stats, (size_t)16));
    A_(dev_alloc(h, &h->d_mt_backup, (size_t)B * kMtN));
    A_(dev_alloc(h, &h->d_pos_backup, (size_t)B));
    A_(dev_alloc(h, &h->d_block_backup, (size_t)B));
    {
        uint32_t *key = nullptr;
        A_(dev_alloc(h, &P.rng_block, (size_t)B));
        A_(dev_alloc(h, &key, (size_t)2 * B));
        P.rng_key = key;
    }
    P.philox = cfg->rng_mode == SMZ_RNG_PHILOX ? 1 : 0;
    h->has_backup = false;
    h->last_kernel[0] = 0;
    if (rc != SMZ_OK) { smz_destroy(h); return rc; }
    P.pbc_sqrt = h->d_pbc;
    P.pow_table = nullptr;
    P.stats = nullptr;
    // defined contents before first use
    hipError_t e = hipMemset(P.nodes, 0, (size_t)B * (size_t)P.tree_words * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(P.hdr, 0, (size_t)B * sizeof(TreeHdr));
    if (e == hipSuccess) e = hipMemset(h->d_stats, 0, 16 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(P.rng_pos, 0, (size_t)B * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(P.mt, 0, (size_t)B * kMtN * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(P.rng_block, 0, (size_t)B * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(const_cast<uint32_t *>(P.rng_key), 0, (size_t)2 * B * sizeof(uint32_t));
    if (e != hipSuccess) { smz_destroy(h); return fail(SMZ_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e)); }
    std::vector<double> tab((size_t)sims + 2);
    for (int n = 0; n < sims + 2; n++)
        tab[n] = log(((double)n + (double)cfg->pb_c_base + 1.0) / (double)cfg->pb_c_base) + cfg->pb_c_init;
    rc = smz_set_pb_c_table(h, tab.data(), sims + 2);
    if (rc != SMZ_OK) { smz_destroy(h); return rc; }
    // default streams: numpy seed(i) for tree i
    std::vector<uint64_t> seeds((size_t)B);
    for (int i = 0; i < B; i++) seeds[i] = (uint64_t)i;
    rc = smz_seed(h, seeds.data(), nullptr);
    if (rc == SMZ_OK) { e = hipDeviceSynchronize(); if (e != hipSuccess) rc = fail(SMZ_ERR_HIP, "sync failed: %s", hipGetErrorString(e)); }
    if (rc != SMZ_OK) { smz_destroy(h); return rc; }
    *out = h;
    return SMZ_OK;
}
}  // namespace

extern "C" {
int smz_destroy(smz_handle *h) {
    if (!h) return SMZ_OK;
    DeviceGuard guard(h->cfg.device);
    (void)hipDeviceSynchronize();
    for (void *p : h->allocs) (void)hipFree(p);
    delete h;
    return SMZ_OK;
}

int smz_set_pb_c_table(smz_handle *h, const double *host_table, int n) {
    if (!h || !host_table) return fail(SMZ_ERR_INVALID, "smz_set_pb_c_table: null argument%s");
    const int need = h->cfg.num_simulations + 2;
    if (n < need) return fail(SMZ_ERR_INVALID, "smz_set_pb_c_table: table shorter than num_simulations + 2%s");
    DeviceGuard guard(h->cfg.device);
    std::vector<double> t((size_t)need);
    for (int i = 0; i < need; i++) t[i] = sqrt((double)i) * host_table[i];  // np.sqrt(Np) * pb_c (mcts:237)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->d_pbc, t.data(), (size_t)need * sizeof(double), hipMemcpyHostToDevice));
    return SMZ_OK;
}

int smz_seed(smz_handle *h, const uint64_t *host_seeds, smz_stream stream) {
    if (!h || !host_seeds) return fail(SMZ_ERR_INVALID, "smz_seed: null argument%s");
    DeviceGuard guard(h->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(s));  // d_seeds may still be read by an earlier smz_seed
    HIP_TRY(hipMemcpy(h->d_seeds, host_seeds, (size_t)h->cfg.num_trees * sizeof(uint64_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_seed, tree_grid(h->P.B), dim3(kWave), 0, s, h->P, h->d_seeds);
    return launch_check();
}

int smz_set_rng_state(smz_handle *h, int tree, const uint32_t *host_key, int pos) {
    if (!h || !host_key || tree < 0 || tree >= h->cfg.num_trees || pos < 0 || pos > kMtN)
        return fail(SMZ_ERR_INVALID, "smz_set_rng_state: bad argument%s");
    if (h->P.philox) return fail(SMZ_ERR_STATE, "smz_set_rng_state: numpy (MT19937) states belong to SMZ_RNG_MT19937_NUMPY handles%s");
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->P.mt + (size_t)tree * kMtN, host_key, kMtN * sizeof(uint32_t), hipMemcpyHostToDevice));
    // numpy block form (all 624 words of the current block, pos consumed) -> incremental form:
    // words pos..623 are already twisted and are handed out as they are.
    const int32_t packed = (pos == kMtN) ? 0 : (((kMtN - pos) << 16) | pos);
    HIP_TRY(hipMemcpy(h->P.rng_pos + tree, &packed, sizeof(int32_t), hipMemcpyHostToDevice));
    return SMZ_OK;
}

int smz_get_rng_state(smz_handle *h, int tree, uint32_t *host_key, int *pos) {
    if (!h || !host_key || !pos || tree < 0 || tree >= h->cfg.num_trees)
        return fail(SMZ_ERR_INVALID, "smz_get_rng_state: bad argument%s");
    if (h->P.philox) return fail(SMZ_ERR_STATE, "smz_get_rng_state: numpy (MT19937) states belong to SMZ_RNG_MT19937_NUMPY handles%s");
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    int32_t packed = 0;
    HIP_TRY(hipMemcpy(host_key, h->P.mt + (size_t)tree * kMtN, kMtN * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&packed, h->P.rng_pos + tree, sizeof(int32_t), hipMemcpyDeviceToHost));
    const int idx = packed & 0xffff, ready = packed >> 16;
    // Device form: words [idx, idx+ready) (cyclic) are twisted ahead of consumption, everything already consumed in
    // this pass is twisted, the rest still holds the previous block.  numpy's form wants one complete block + pos.
    auto twist_at = [&](int i) {
        const int i1 = (i + 1 == kMtN) ? 0 : i + 1;
        int im = i + kMtM;
        if (im >= kMtN) im -= kMtN;
        const uint32_t t = (host_key[i] & 0x80000000u) | (host_key[i1] & 0x7fffffffu);
        host_key[i] = host_key[im] ^ (t >> 1) ^ ((t & 1u) ? 0x9908b0dfu : 0u);
    };
    if (idx + ready <= kMtN) {
        if (idx == 0 && ready == 0) { *pos = kMtN; return SMZ_OK; }   // block boundary: numpy regenerates next
        for (int i = idx + ready; i < kMtN; i++) twist_at(i);          // finish the in-place pass
        *pos = idx;
        return SMZ_OK;
    }
    // The twist-ahead window wrapped: words [0, w) already hold NEXT-block values.  Recover the current-block words
    // they replaced by inverting the twist (new[k] ^ cur[k+397] gives the msb of cur[k] and the low 31 bits of
    // cur[k+1]; the low bits of cur[0] are never read again by the generator and are left zero).
    const int w = idx + ready - kMtN;
    if (w + kMtM > kMtN) return fail(SMZ_ERR_STATE, "smz_get_rng_state: twist-ahead window too long%s");
    std::vector<uint32_t> t((size_t)w);
    for (int k = 0; k < w; k++) {
        uint32_t y = host_key[k] ^ host_key[k + kMtM];
        uint32_t low = 0;
        if (y & 0x80000000u) { y ^= 0x9908b0dfu; low = 1u; }
        t[k] = (y << 1) | low;                                       // (cur[k] & UPPER) | (cur[k+1] & LOWER)
    }
    for (int k = 0; k < w; k++)
        host_key[k] = (t[k] & 0x80000000u) | (k > 0 ? (t[k - 1] & 0x7fffffffu) : 0u);
    *pos = idx;
    return SMZ_OK;
}

int smz_rng_snapshot(smz_handle *h, smz_stream stream) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_rng_snapshot: null handle%s");
    DeviceGuard guard(h->cfg.device);
    const size_t B = (size_t)h->cfg.num_trees;
    HIP_TRY(hipMemcpyAsync(h->d_mt_backup, h->P.mt, B * kMtN * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(h->d_pos_backup, h->P.rng_pos, B * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(h->d_block_backup, h->P.rng_block, B * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    h->has_backup = true;
    return SMZ_OK;
}

int smz_rng_restore(smz_handle *h, smz_stream stream) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_rng_restore: null handle%s");
    if (!h->has_backup) return fail(SMZ_ERR_STATE, "smz_rng_restore without smz_rng_snapshot%s");
    DeviceGuard guard(h->cfg.device);
    const size_t B = (size_t)h->cfg.num_trees;
    HIP_TRY(hipMemcpyAsync(h->P.mt, h->d_mt_backup, B * kMtN * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(h->P.rng_pos, h->d_pos_backup, B * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(h->P.rng_block, h->d_block_backup, B * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SMZ_OK;
}

int smz_root_init(smz_handle *h, const float *hidden_dev, const float *policy_dev, const double *noise_override_dev,
                  int train, smz_stream stream) {
    if (!h || !policy_dev) return fail(SMZ_ERR_INVALID, "smz_root_init: null argument%s");
    if (h->P.S > 0 && !hidden_dev) return fail(SMZ_ERR_INVALID, "smz_root_init: hidden_dev is required when hidden_size > 0%s");
    if (train && h->cfg.num_simulations > 0 && !(h->cfg.root_dirichlet_alpha > 0))
        return fail(SMZ_ERR_INVALID, "root_dirichlet_alpha must be > 0 to draw noise (numpy raises ValueError)%s");
    DeviceGuard guard(h->cfg.device);
    if (h->large_actions) {
        h->root_ready = true;
        h->selected = false;
        return smz_internal_la_root_init(h, hidden_dev, policy_dev, noise_override_dev, train, stream);
    }
    SMZ_DISPATCH(h->maxa, hipLaunchKernelGGL((k_root_init<MA>), wave_grid(h->P), dim3(kWave), tree_lds_bytes(h->P), (hipStream_t)stream,
                                             h->P, hidden_dev, policy_dev, noise_override_dev, train));
    h->root_ready = true;
    h->selected = false;
    return launch_check();
}

int smz_select(smz_handle *h, float *parent_hidden_dev, int32_t *last_action_dev, uint8_t *branch_dev,
               float *mlp_input_dev, smz_stream stream) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_select: null handle%s");
    if (!h->root_ready) return fail(SMZ_ERR_STATE, "smz_select before smz_root_init%s");
    DeviceGuard guard(h->cfg.device);
    if (h->large_actions) {
        h->selected = true;
        return smz_internal_la_select(h, parent_hidden_dev, last_action_dev, branch_dev, mlp_input_dev, stream);
    }
    SMZ_DISPATCH2_AEX(h->maxa, h->K, h->P.A == h->maxa && !h->P.philox, hipLaunchKernelGGL((k_select<MA, KS, AEX>), wave_grid(h->P), dim3(kWave), tree_lds_bytes(h->P), (hipStream_t)stream, h->P,
                                             parent_hidden_dev, last_action_dev, branch_dev, mlp_input_dev));
    h->selected = true;
    return launch_check();
}

int smz_expand_backup(smz_handle *h, const float *hidden_dev, const float *reward_dev, const float *policy_dev,
                      const float *value_dev, smz_stream stream) {
    if (!h || !policy_dev || !value_dev) return fail(SMZ_ERR_INVALID, "smz_expand_backup: null argument%s");
    if (!h->selected) return fail(SMZ_ERR_STATE, "smz_expand_backup without a preceding smz_select%s");
    DeviceGuard guard(h->cfg.device);
    if (h->large_actions) {
        h->selected = false;
        return smz_internal_la_expand_backup(h, hidden_dev, reward_dev, policy_dev, value_dev, stream);
    }
    if (h->P.n_cycle > 1) {     // multi-player handle (smz_set_players)
        SMZ_DISPATCH2_AEX(h->maxa, h->K, h->P.A == h->maxa && !h->P.philox, hipLaunchKernelGGL((k_expand_backup_mp<MA, KS, false, AEX>), wave_grid(h->P), dim3(kWave), tree_lds_bytes(h->P),
                                                 (hipStream_t)stream, h->P, hidden_dev, reward_dev, policy_dev, value_dev,
                                                 (float *)nullptr, (int32_t *)nullptr, (uint8_t *)nullptr, (float *)nullptr));
    } else {
        SMZ_DISPATCH2_AEX(h->maxa, h->K, h->P.A == h->maxa && !h->P.philox, hipLaunchKernelGGL((k_expand_backup<MA, KS, false, AEX>), wave_grid(h->P), dim3(kWave), tree_lds_bytes(h->P),
                                                 (hipStream_t)stream, h->P, hidden_dev, reward_dev, policy_dev, value_dev,
                                                 (float *)nullptr, (int32_t *)nullptr, (uint8_t *)nullptr, (float *)nullptr));
    }
    h->selected = false;
    return launch_check();
}

int smz_root_stats(smz_handle *h, int32_t *visits_dev, double *priors_dev, float *root_value_dev,
                   float *child_reward_dev, smz_stream stream) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_root_stats: null handle%s");
    if (!h->root_ready) return fail(SMZ_ERR_STATE, "smz_root_stats before smz_root_init%s");
    DeviceGuard guard(h->cfg.device);
    hipLaunchKernelGGL(k_root_stats, tree_grid(h->P.B), dim3(kWave), 0, (hipStream_t)stream, h->P, visits_dev, priors_dev,
                       root_value_dev, child_reward_dev);
    return launch_check();
}

int smz_act(smz_handle *h, double temperature, const double *pow_table_host, int32_t *action_dev, double *policy_dev,
            double *child_visits_dev, float *root_value_dev, smz_stream stream) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_act: null handle%s");
    if (!h->root_ready) return fail(SMZ_ERR_STATE, "smz_act before smz_root_init%s");
    DeviceGuard guard(h->cfg.device);
    Params P = h->P;
    if (use_pow_table(h, P, temperature, pow_table_host, stream) != SMZ_OK) return SMZ_ERR_HIP;
    if (h->large_actions) return smz_internal_la_act(h, P, temperature, action_dev, policy_dev, child_visits_dev, root_value_dev, stream);
    SMZ_DISPATCH(h->maxa, hipLaunchKernelGGL((k_act<MA>), tree_grid(P.B), dim3(kWave), 0, (hipStream_t)stream, P, temperature,
                                             action_dev, policy_dev, child_visits_dev, root_value_dev));
    return launch_check();
}

int smz_support_decode(const float *logits_dev, int S, float *out_dev, int B, smz_stream stream) {
    if (!logits_dev || !out_dev || S < 1 || B < 1) return fail(SMZ_ERR_INVALID, "smz_support_decode: bad argument%s");
    const int lpr = group_lanes(S);
    hipLaunchKernelGGL(k_support_decode, group_grid(B, lpr), dim3(256), 0, (hipStream_t)stream, logits_dev, S, out_dev, B, lpr);
    return launch_check();
}

int smz_policy_softmax(const float *logits_dev, int A, float *out_dev, int B, smz_stream stream) {
    if (!logits_dev || !out_dev || A < 1 || B < 1) return fail(SMZ_ERR_INVALID, "smz_policy_softmax: bad argument%s");
    const int lpr = group_lanes(A);
    hipLaunchKernelGGL(k_policy_softmax, group_grid(B, lpr), dim3(256), 0, (hipStream_t)stream, logits_dev, A, out_dev, B, lpr);
    return launch_check();
}

int smz_dynamics_epilogue(const float *state_dyn_dev, const float *state_after_dev, const float *reward_logits_dev,
                          int ld, const uint8_t *branch_dev, int S, float *hidden_out_dev, float *reward_out_dev, int B,
                          smz_stream stream) {
    if (!state_dyn_dev || !state_after_dev || !branch_dev || !hidden_out_dev || S < 1 || B < 1 || ld < S)
        return fail(SMZ_ERR_INVALID, "smz_dynamics_epilogue: bad argument%s");
    const int lpr = group_lanes(S);
    hipLaunchKernelGGL(k_dynamics_epilogue, group_grid(B, lpr), dim3(256), 0, (hipStream_t)stream, state_dyn_dev,
                       state_after_dev, reward_logits_dev, ld, branch_dev, S, hidden_out_dev, reward_out_dev, B, lpr);
    return launch_check();
}

int smz_prediction_epilogue(const float *policy_logits_pred_dev, const float *value_logits_pred_dev,
                            const float *policy_logits_after_dev, const float *value_logits_after_dev,
                            int ld, const uint8_t *branch_dev, int A, int S, float *policy_out_dev,
                            float *value_out_dev, int B, smz_stream stream) {
    if (!policy_logits_pred_dev || !value_logits_pred_dev || !policy_logits_after_dev || !value_logits_after_dev ||
        !branch_dev || !policy_out_dev || !value_out_dev || A < 1 || S < 1 || B < 1 || ld < 1)
        return fail(SMZ_ERR_INVALID, "smz_prediction_epilogue: bad argument%s");
    const int lpr = group_lanes(S > A ? S : A);
    hipLaunchKernelGGL(k_prediction_epilogue, group_grid(B, lpr), dim3(256), 0, (hipStream_t)stream, policy_logits_pred_dev,
                       value_logits_pred_dev, policy_logits_after_dev, value_logits_after_dev, ld, branch_dev, A, S,
                       policy_out_dev, value_out_dev, B, lpr);
    return launch_check();
}

int smz_cartpole_step(double *state_dev, const int32_t *action_dev, float *obs_out_dev, float *reward_out_dev,
                      uint8_t *terminated_out_dev, int B, smz_stream stream) {
    if (!state_dev || !action_dev || B < 1) return fail(SMZ_ERR_INVALID, "smz_cartpole_step: bad argument%s");
    const EnvStep E = {state_dev, obs_out_dev, reward_out_dev, terminated_out_dev, nullptr, nullptr, nullptr, 0, 0, 0, 0, nullptr, 0};
    hipLaunchKernelGGL(k_cartpole_step_env, row_grid(B), dim3(256), 0, (hipStream_t)stream, E, action_dev, B,
                       (const double *)nullptr, (const double *)nullptr, (const float *)nullptr);
    return launch_check();
}

int smz_cartpole_step_pack(double *state_dev, const int32_t *action_dev, float *obs_out_dev, float *reward_out_dev,
                           uint8_t *terminated_out_dev, double *traj_dev, int T, int t, const double *policy_dev,
                           const double *child_visits_dev, const float *root_value_dev, int B, smz_stream stream) {
    if (!state_dev || !action_dev || !traj_dev || !policy_dev || !child_visits_dev || !root_value_dev || t < 0 || t >= T || B < 1)
        return fail(SMZ_ERR_INVALID, "smz_cartpole_step_pack: bad argument%s");
    const EnvStep E = {state_dev, obs_out_dev, reward_out_dev, terminated_out_dev, nullptr, nullptr, nullptr, 0, 0, 0, 0, traj_dev, t};
    hipLaunchKernelGGL(k_cartpole_step_env, row_grid(B), dim3(256), 0, (hipStream_t)stream, E, action_dev, B, policy_dev,
                       child_visits_dev, root_value_dev);
    return launch_check();
}

int smz_cartpole_step_ctl(double *state_dev, const int32_t *action_dev, float *obs_out_dev, float *reward_out_dev,
                          uint8_t *flag_out_dev, const smz_episode_ctl *ctl, double *traj_dev, int T, int t,
                          const double *policy_dev, const double *child_visits_dev, const float *root_value_dev, int B,
                          smz_stream stream) {
    if (!state_dev || !action_dev || !ctl || B < 1) return fail(SMZ_ERR_INVALID, "smz_cartpole_step_ctl: bad argument%s");
    if (!episode_ctl_ok("smz_cartpole_step_ctl", ctl)) return SMZ_ERR_INVALID;
    if (traj_dev && (!policy_dev || !child_visits_dev || !root_value_dev || t < 0 || t >= T))
        return fail(SMZ_ERR_INVALID, "smz_cartpole_step_ctl: bad trajectory argument%s");
    const EnvStep E = {state_dev, obs_out_dev, reward_out_dev, flag_out_dev, ctl->step_count_dev, ctl->episode_dev,
                       ctl->active_dev, ctl->limit, ctl->on_end, (uint64_t)ctl->reset_seed, (long long)ctl->first_env, traj_dev, t};
    hipLaunchKernelGGL(k_cartpole_step_env, row_grid(B), dim3(256), 0, (hipStream_t)stream, E, action_dev, B, policy_dev,
                       child_visits_dev, root_value_dev);
    return launch_check();
}

int smz_cartpole_reset_state(uint64_t reset_seed, int64_t env, int64_t episode, double state_out[4]) {
    if (!state_out || episode < 1) return fail(SMZ_ERR_INVALID, "smz_cartpole_reset_state: bad argument%s");
    for (int c = 0; c < 4; c++) state_out[c] = -0.05 + 0.1 * smz_unit(reset_seed, (uint64_t)env, (uint64_t)episode, (uint64_t)c);
    return SMZ_OK;
}

int smz_host_cartpole_step(double *state_host, const int32_t *action_host, float *obs_out_host, float *reward_out_host,
                           uint8_t *flag_out_host, int32_t *step_count_host, int32_t limit, int B) {
    if (!state_host || !action_host || B < 1) return fail(SMZ_ERR_INVALID, "smz_host_cartpole_step: bad argument%s");
    const double g = 9.8, mc = 1.0, mp = 0.1, tm = mc + mp, len = 0.5, pml = mp * len, fm = 10.0, tau = 0.02;
    for (int e = 0; e < B; e++) {
        double *st = state_host + (size_t)e * 4;
        const double x = st[0], xd = st[1], th = st[2], thd = st[3];
        const double force = action_host[e] == 1 ? fm : -fm;
        const double ct = cos(th), sn = sin(th);
        const double temp = (force + pml * thd * thd * sn) / tm;
        const double tha = (g * sn - ct * temp) / (len * (4.0 / 3.0 - mp * ct * ct / tm));
        const double xa = temp - pml * tha * ct / tm;
        const double nx = x + tau * xd, nxd = xd + tau * xa, nth = th + tau * thd, nthd = thd + tau * tha;
        st[0] = nx; st[1] = nxd; st[2] = nth; st[3] = nthd;
        if (obs_out_host) {
            float *o = obs_out_host + (size_t)e * 4;
            o[0] = (float)nx; o[1] = (float)nxd; o[2] = (float)nth; o[3] = (float)nthd;
        }
        if (reward_out_host) reward_out_host[e] = 1.0f;
        const bool term = fabs(nx) > 2.4 || fabs(nth) > 12.0 * 2.0 * 3.14159265358979323846 / 360.0;
        int flag = term ? 1 : 0;
        if (step_count_host) {
            const int count = ++step_count_host[e];
            if (limit > 0 && count == limit) flag = 2;
        }
        if (flag_out_host) flag_out_host[e] = (uint8_t)flag;
    }
    return SMZ_OK;
}

int smz_synthetic_obs(float *obs_dev, int B, int obs_dim, uint64_t seed, int64_t first_env, int64_t t, smz_stream stream) {
    if (!obs_dev || B < 1 || obs_dim < 1) return fail(SMZ_ERR_INVALID, "smz_synthetic_obs: bad argument%s");
    const size_t n = (size_t)B * obs_dim;
    hipLaunchKernelGGL(k_synthetic_obs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, obs_dev, B,
                       obs_dim, seed, (long long)first_env, (long long)t);
    return launch_check();
}

int smz_set_active(smz_handle *h, const uint8_t *active_dev) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_set_active: null handle%s");
    h->P.active = active_dev;
    return SMZ_OK;
}

int smz_set_players(smz_handle *h, int n_cycle, const float *cycle_values_host, const int32_t *root_player_dev) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_set_players: null handle%s");
    if (n_cycle < 1 || n_cycle > SMZ_MAX_PLAYER_CYCLE)
        return fail(SMZ_ERR_INVALID, "smz_set_players: the turn cycle must have 1 .. SMZ_MAX_PLAYER_CYCLE (32) entries%s");
    if (n_cycle > 1 && !cycle_values_host) return fail(SMZ_ERR_INVALID, "smz_set_players: null cycle_values_host%s");
    if (n_cycle == 1) {          // one player: every backed-up value keeps its sign -- the plain kernels
        h->P.n_cycle = 1;
        h->P.root_player = nullptr;
        return SMZ_OK;
    }
    uint32_t neg[SMZ_MAX_PLAYER_CYCLE] = {0u};
    for (int r = 0; r < n_cycle; r++)
        for (int j = 0; j < n_cycle; j++)
            if (!(cycle_values_host[r] == cycle_values_host[(r + j) % n_cycle])) neg[r] |= 1u << j;
    DeviceGuard guard(h->cfg.device);
    if (!h->d_player_neg) {
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, SMZ_MAX_PLAYER_CYCLE * sizeof(uint32_t)));
        h->allocs.push_back(p);
        h->d_player_neg = (uint32_t *)p;
    }
    // (synchronous: kernels already enqueued on any stream have read the previous table)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->d_player_neg, neg, sizeof(neg), hipMemcpyHostToDevice));
    h->P.player_neg = h->d_player_neg;
    h->P.n_cycle = n_cycle;
    h->P.root_player = root_player_dev;
    return SMZ_OK;
}

int smz_set_leaf_ids_out(smz_handle *h, int32_t *ids_dev) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_set_leaf_ids_out: null handle%s");
    h->P.ids_out = ids_dev;
    return SMZ_OK;
}

int smz_get_hidden_layout(smz_handle *h, float **hidden_dev_out, int *nodes_per_tree_out, int *row_stride_out) {
    if (!h || !hidden_dev_out || !nodes_per_tree_out || !row_stride_out) return fail(SMZ_ERR_INVALID, "smz_get_hidden_layout: null argument%s");
    *hidden_dev_out = h->P.hidden;
    *nodes_per_tree_out = h->P.N;
    *row_stride_out = h->P.hs;
    return SMZ_OK;
}

int smz_traj_floats(int obs_dim, int A) { return obs_dim + 3 * A + 3; }

int smz_traj_pack(double *traj_dev, int T, int t, int obs_dim, int A, const float *obs_dev, const float *reward_dev,
                  const uint8_t *terminated_dev, const int32_t *action_dev, const double *policy_dev, const double *child_visits_dev,
                  const float *root_value_dev, int B, smz_stream stream) {
    if (!traj_dev || (!obs_dev && obs_dim > 0) || !action_dev || !policy_dev || !child_visits_dev || !root_value_dev || t < 0 ||
        t >= T || B < 1 || A < 1 || obs_dim < 0)
        return fail(SMZ_ERR_INVALID, "smz_traj_pack: bad argument%s");
    const size_t slab = (size_t)B * (obs_dim + 3 * A + 3);
    const unsigned blocks = (unsigned)std::min<size_t>((slab + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(k_traj_pack, dim3(blocks), dim3(256), 0, (hipStream_t)stream, traj_dev, T, t, obs_dim, A, obs_dev,
                       reward_dev, terminated_dev, action_dev, policy_dev, child_visits_dev, root_value_dev, B);
    return launch_check();
}

int smz_traj_targets(const double *traj_dev, int T, int obs_dim, int A, int B, int td_steps, const double *discount_pow_dev,
                     int ignore_termination, int32_t *length_dev, double *value_target_dev, double *abs_td_error_dev,
                     smz_stream stream) {
    if (!traj_dev || !discount_pow_dev || !length_dev || !value_target_dev || T < 1 || B < 1 || A < 1 || obs_dim < 0 ||
        td_steps < 0)
        return fail(SMZ_ERR_INVALID, "smz_traj_targets: bad argument%s");
    hipLaunchKernelGGL(k_traj_lengths, row_grid(B), dim3(256), 0, (hipStream_t)stream, traj_dev, T, obs_dim, A, B,
                       ignore_termination, length_dev);
    const size_t cells = (size_t)T * B;
    hipLaunchKernelGGL(k_traj_targets, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, traj_dev, T,
                       obs_dim, A, B, td_steps, discount_pow_dev, (const int32_t *)length_dev, value_target_dev,
                       abs_td_error_dev, (const int32_t *)nullptr);
    return launch_check();
}

int smz_traj_targets_games(const double *traj_dev, int T, int obs_dim, int A, int B, int td_steps,
                           const double *discount_pow_dev, int ignore_termination, int new_game, int32_t *length_dev,
                           int32_t *game_end_dev, double *value_target_dev, double *abs_td_error_dev, smz_stream stream) {
    if (!traj_dev || !discount_pow_dev || !game_end_dev || !value_target_dev || T < 1 || B < 1 || A < 1 || obs_dim < 0 ||
        td_steps < 0)
        return fail(SMZ_ERR_INVALID, "smz_traj_targets_games: bad argument%s");
    hipLaunchKernelGGL(k_traj_game_ends, row_grid(B), dim3(256), 0, (hipStream_t)stream, traj_dev, T, obs_dim, A, B,
                       ignore_termination, new_game, length_dev, game_end_dev);
    const size_t cells = (size_t)T * B;
    hipLaunchKernelGGL(k_traj_targets, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, traj_dev, T,
                       obs_dim, A, B, td_steps, discount_pow_dev, (const int32_t *)nullptr, value_target_dev, abs_td_error_dev,
                       (const int32_t *)game_end_dev);
    return launch_check();
}

int smz_debug_div_by_count(const double *x_dev, const int32_t *n_dev, int count, int table_size, double *out_dev,
                           smz_stream stream) {
    if (!x_dev || !n_dev || !out_dev || count < 1 || table_size < 2 || table_size > kPbcLdsMax)
        return fail(SMZ_ERR_INVALID, "smz_debug_div_by_count: bad argument%s");
    hipLaunchKernelGGL(k_debug_div_by_count, dim3(256), dim3(256), (size_t)table_size * sizeof(double), (hipStream_t)stream,
                       x_dev, n_dev, count, table_size, out_dev);
    return launch_check();
}

int smz_debug_glibc_log_pow(const double *x_dev, const double *y_dev, int count, double *out_log_dev, double *out_pow_dev,
                            smz_stream stream) {
    if (!x_dev || count < 1 || (!out_log_dev && !out_pow_dev) || (out_pow_dev && !y_dev))
        return fail(SMZ_ERR_INVALID, "smz_debug_glibc_log_pow: bad argument%s");
    hipLaunchKernelGGL(k_debug_glibc_log_pow, dim3(1024), dim3(256), 0, (hipStream_t)stream, x_dev, y_dev, count, out_log_dev,
                       out_pow_dev);
    return launch_check();
}

int smz_debug_dump_tree(smz_handle *h, int tree, smz_node_view *nodes, int cap, float *minmax_out, int32_t *path_out,
                        int cap_path, int32_t *path_len_out, double *root_priors_out) {
    if (!h || tree < 0 || tree >= h->cfg.num_trees) return fail(SMZ_ERR_INVALID, "smz_debug_dump_tree: bad argument%s");
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    const Params &P = h->P;
    const int A = P.A, K = P.K;
    TreeHdr hdr;
    HIP_TRY(hipMemcpy(&hdr, P.hdr + tree, sizeof(hdr), hipMemcpyDeviceToHost));
    std::vector<uint32_t> blob((size_t)P.tree_words);
    HIP_TRY(hipMemcpy(blob.data(), P.nodes + (size_t)tree * P.tree_words, (size_t)P.tree_words * 4, hipMemcpyDeviceToHost));
    const int n = 1 + A + hdr.n_exp * K;
    auto f32 = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
    if (nodes && cap > 0) {
        // flatten the child blocks back to creation-order node ids (root 0, its children 1..A, expansion e at 1+A+e*K)
        if (cap > 0) nodes[0] = smz_node_view{hdr.root_visit, hdr.root_value_sum, 0.f, 0.f, 1, 0};
        for (int a = 0; a < A && 1 + a < cap; a++) {
            const uint32_t *rb = blob.data();
            const int c = (int)rb[4 * A + a];
            nodes[1 + a] = smz_node_view{(int32_t)rb[2 * a], f32(rb[2 * a + 1]), f32(rb[2 * A + a]), f32(rb[3 * A + a]),
                                         c ? 1 + A + (c - 1) * K : 0, a};
        }
        for (int e = 0; e < hdr.n_exp; e++) {
            const uint32_t *eb = blob.data() + P.rb_words + (size_t)e * P.eb_words;
            for (int j = 0; j < K; j++) {
                const int id = 1 + A + e * K + j;
                if (id >= cap) break;
                const int c = (int)eb[4 * K + j];
                nodes[id] = smz_node_view{(int32_t)eb[2 * j], f32(eb[2 * j + 1]), f32(eb[2 * K + j]), f32(eb[3 * K + j]),
                                          c ? 1 + A + (c - 1) * K : 0, (int32_t)eb[5 * K + j]};
            }
        }
    }
    if (minmax_out) { minmax_out[0] = hdr.mn; minmax_out[1] = hdr.mx; }
    // the recorded path as node ids, root first (the device stores (block << 8 | slot) without the root)
    const int plen = hdr.path_len > 0 ? hdr.path_len + 1 : 0;
    if (path_len_out) *path_len_out = plen;
    if (path_out && cap_path > 0 && plen > 0) {
        std::vector<uint4> recs((size_t)hdr.path_len);
        HIP_TRY(hipMemcpy2D(recs.data(), sizeof(uint4), P.path + tree, (size_t)P.B * sizeof(uint4), sizeof(uint4), (size_t)hdr.path_len, hipMemcpyDeviceToHost));
        path_out[0] = 0;
        const int sb = h->large_actions ? 10 : 8;          // slot bits of a path record (smz_large_actions.hip: kLaSlotBits)
        for (int i = 0; i < hdr.path_len && i + 1 < cap_path; i++) {
            const int blk = (int)recs[i].x >> sb, slot = (int)recs[i].x & ((1 << sb) - 1);
            path_out[i + 1] = blk == 0 ? 1 + slot : 1 + A + (blk - 1) * K + slot;
        }
    }
    if (root_priors_out) memcpy(root_priors_out, blob.data() + P.rp_off, (size_t)A * 8);
    return n;
}

int smz_philox_words(uint64_t seed, uint32_t block, int idx, int n, uint32_t *host_out) {
    if (!host_out || n < 0 || idx < 0 || idx >= kMtN) return fail(SMZ_ERR_INVALID, "smz_philox_words: bad argument%s");
    for (int i = 0; i < n; i++) {
        host_out[i] = philox_word(block, idx, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
        if (++idx == kMtN) { idx = 0; ++block; }
    }
    return SMZ_OK;
}

int smz_get_philox_position(smz_handle *h, int tree, uint32_t *block_out, int *idx_out) {
    if (!h || tree < 0 || tree >= h->cfg.num_trees || !block_out || !idx_out)
        return fail(SMZ_ERR_INVALID, "smz_get_philox_position: bad argument%s");
    if (!h->P.philox) return fail(SMZ_ERR_STATE, "smz_get_philox_position: the handle draws from MT19937%s");
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    int32_t packed = 0;
    HIP_TRY(hipMemcpy(&packed, h->P.rng_pos + tree, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(block_out, h->P.rng_block + tree, sizeof(uint32_t), hipMemcpyDeviceToHost));
    *idx_out = packed & 0xffff;
    return SMZ_OK;
}

int smz_enable_stats(smz_handle *h, int on) {
    if (!h) return fail(SMZ_ERR_INVALID, "smz_enable_stats: null handle%s");
    if (h->large_actions && on)
        return fail(SMZ_ERR_TOO_LARGE, "smz_enable_stats: the large-action kernels keep no level statistics%s");
    h->stats_on = on != 0;
    h->P.stats = h->stats_on ? h->d_stats : nullptr;
    return SMZ_OK;
}

int smz_read_stats(smz_handle *h, uint64_t levels_out[4], int reset) {
    if (!h || !levels_out) return fail(SMZ_ERR_INVALID, "smz_read_stats: null argument%s");
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v[16];
    HIP_TRY(hipMemcpy(v, h->d_stats, sizeof(v), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++) levels_out[i] = (uint64_t)v[i];
    if (getenv("SMZ_DEBUG_SKIP") && (atoi(getenv("SMZ_DEBUG_SKIP")) & 16))
        fprintf(stderr, "[smz phase cycles, summed over waves] stage %llu expand %llu select %llu mlp %llu  (k_search_vision: tree, conv, wait, towers+tails)\n", v[4], v[5], v[6], v[7]);
#ifdef SMZ_BPS_PROBE
    if (v[8])
        fprintf(stderr, "[smz k_search_mlp probe, cycles summed over waves] expand+backup %llu | select: prepare %llu evaluate %llu chase %llu records+leaf %llu "
                        "| networks %llu | staging %llu\n", v[8], v[9], v[10], v[11], v[12], v[13], v[14]);
#endif
    if (getenv("SMZ_DEBUG_SKIP") && (atoi(getenv("SMZ_DEBUG_SKIP")) & 16) && v[8])
        fprintf(stderr, "[smz k_search_vision phases] tree %llu load %llu conv_transition %llu conv_prediction %llu wait %llu layer1 %llu hidden_out %llu tails_stage %llu\n",
                v[8], v[9], v[10], v[11], v[12], v[13], v[14], v[15]);
    if (reset) HIP_TRY(hipMemset(h->d_stats, 0, sizeof(v)));
    return SMZ_OK;
}

}  // extern "C"
