// smz_handle.hpp -- host side shared by the translation units of libsmz.so: the handle, the last-error text, launch helpers
// and the host path the single-launch searches share.
#pragma once
#include "smz_common.hpp"

struct smz_handle {
    smz_config cfg;
    Params P;
    int K, N, Ppath;
    int maxa;  // template bucket
    bool root_ready, selected;
    uint64_t *d_seeds;
    double *d_pbc;
    double *d_pow;
    double pow_T;
    bool pow_valid;
    unsigned long long *d_stats;
    bool stats_on;
    uint32_t *d_mt_backup;
    int32_t *d_pos_backup;
    uint32_t *d_block_backup;
    bool has_backup;
    std::vector<void *> allocs;
    char last_kernel[96];      // the single-launch search instantiation launched last, as rocprofv3 prints it (smz_last_kernel)
    uint32_t *d_player_neg;    // [SMZ_MAX_PLAYER_CYCLE] sign masks of smz_set_players (allocated by its first multi-player call)
    bool large_actions;        // smz_create_large_actions: the step-wise calls run the wave-per-tree kernels (smz_large_actions.hip)
    float *d_la_policy;        // [B][A] policy work rows of smz_search_mlp_large (allocated by its first call)
};

// the last-error text: defined in smz_kernels.hip
extern thread_local char smz_g_err[512];
#define g_err smz_g_err

namespace {

int fail(int code, const char *fmt, const char *detail = "") {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            snprintf(g_err, sizeof(g_err), "%s failed: %s", #expr, hipGetErrorString(e_)); \
            return SMZ_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

template <typename T>
int dev_alloc(smz_handle *h, T **out, size_t count) {
    void *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
        return SMZ_ERR_NOMEM;
    }
    h->allocs.push_back(p);
    *out = (T *)p;
    return SMZ_OK;
}

inline dim3 tree_grid(int B) { return dim3((unsigned)((B + kWave - 1) / kWave)); }
inline dim3 wave_grid(const Params &P) { return dim3((unsigned)((P.B + P.tpw - 1) / P.tpw)); }
inline size_t tree_lds_bytes(const Params &P) {
    static const size_t pad = getenv("SMZ_DEBUG_LDS_PAD") ? (size_t)atoi(getenv("SMZ_DEBUG_LDS_PAD")) : 0;   // occupancy experiments
    return ((P.sims + 2 <= kPbcLdsMax) ? (size_t)(P.sims + 2) * sizeof(double) : 0) +
           (P.lds_stage ? (size_t)kWave * kRngStride * sizeof(uint32_t) : 0) + pad;
}
inline dim3 row_grid(int B) { return dim3((unsigned)((B + 255) / 256)); }
inline int group_lanes(int width) { int l = 1; while (l < width && l < kWave) l <<= 1; return l; }
inline dim3 group_grid(int B, int lpr) { const int per = 256 / lpr; return dim3((unsigned)((B + per - 1) / per)); }

int launch_check() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "kernel launch failed: %s", hipGetErrorString(e));
        return SMZ_ERR_HIP;
    }
    return SMZ_OK;
}

// What every entry point that takes a smz_episode_ctl (non-null) requires of it; the refusal is in the last-error text.
bool episode_ctl_ok(const char *who, const smz_episode_ctl *c) {
    if (c->step_count_dev && c->on_end >= 0 && c->on_end <= 2 && !(c->on_end == 2 && !c->episode_dev) &&
        !(c->on_end == 1 && !c->active_dev))
        return true;
    fail(SMZ_ERR_INVALID, "%s: bad smz_episode_ctl: it needs step_count_dev, on_end 1 needs active_dev, on_end 2 needs episode_dev", who);
    return false;
}

// ---- the host path the single-launch searches share ----
// Refusals that are word for word the same in every search; `who` is the entry point or launcher the message names.
int refuse_large_actions(const char *who) { return fail(SMZ_ERR_TOO_LARGE, "%s: large-action handles search step-wise only", who); }
int refuse_multi_player(const char *who) { return fail(SMZ_ERR_INVALID, "%s: multi-player handles search step-wise only", who); }
int check_dirichlet_alpha(const smz_handle *h, int train) {
    if (train && h->cfg.num_simulations > 0 && !(h->cfg.root_dirichlet_alpha > 0))
        return fail(SMZ_ERR_INVALID, "root_dirichlet_alpha must be > 0 to draw noise (numpy raises ValueError)%s");
    return SMZ_OK;
}

// Trees per wavefront: every one of `waves` wavefronts (the launcher's workgroups per CU x kCus x wavefronts per workgroup) has a
// tree before any takes a second one.  The environment variable `env_override` (nullptr: none) replaces the count (tests: a
// search does not depend on the geometry).
int single_launch_tpw(int B, int waves, const char *env_override) {
    int tpw = (B + waves - 1) / waves;
    if (const char *e = env_override ? getenv(env_override) : nullptr) {
        const int v = atoi(e);
        if (v >= 1) tpw = v;
    }
    return tpw < 1 ? 1 : tpw;
}
// The two size limits of a single-launch kernel: a tree per lane, and an LDS map of `lds_floats` floats on one CU.
int check_single_launch_size(const char *who, int tpw, long long lds_floats) {
    if (tpw > kWave) return fail(SMZ_ERR_TOO_LARGE, "%s: more than 64 trees per wavefront: use the step-wise entry points", who);
    if (lds_floats * (long long)sizeof(float) > 160 * 1024)
        return fail(SMZ_ERR_TOO_LARGE, "%s: working set exceeds the 160 KB LDS of a CU", who);
    return SMZ_OK;
}
// The entry points that only search, and what the `_act` entry points require of their outputs (root_value may be null).
constexpr ActOut kNoAct = {0.0, nullptr, nullptr, nullptr, nullptr};
int check_act_outputs(const char *who, const int32_t *action_dev, const double *policy_dev, const double *child_visits_dev) {
    if (!action_dev || !policy_dev || !child_visits_dev) return fail(SMZ_ERR_INVALID, "%s: null output", who);
    return SMZ_OK;
}

// The power table of `temperature` for act_tree (smz_act, and the searches that act in their tail): a new temperature is a
// synchronous upload (not capturable); the table is reused while the temperature is unchanged.
int use_pow_table(smz_handle *h, Params &P, double temperature, const double *pow_table_host, smz_stream stream) {
    if (!pow_table_host || !(temperature >= 0.3)) return SMZ_OK;
    if (!h->pow_valid || h->pow_T != temperature) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        HIP_TRY(hipMemcpy(h->d_pow, pow_table_host, ((size_t)h->cfg.num_simulations + 1) * sizeof(double), hipMemcpyHostToDevice));
        h->pow_T = temperature;
        h->pow_valid = true;
    }
    P.pow_table = h->d_pow;
    return SMZ_OK;
}

// Launches the instantiation `Kern` with `lds` bytes of dynamic LDS.  The opt-in above the default limit is a host-side call:
// made once per instantiation and device, and again only when a launch needs more.
template <auto Kern, class... Args>
int launch_with_lds(smz_handle *h, int blocks, int threads, size_t lds, smz_stream stream, Args... args) {
    static size_t granted_dev[64] = {};
    size_t &granted = granted_dev[h->cfg.device & 63];
    if (lds > granted) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(SMZ_ERR_HIP, "hipFuncSetAttribute(max dynamic LDS) failed%s");
        granted = lds;
    }
    hipLaunchKernelGGL(Kern, dim3(blocks), dim3(threads), lds, (hipStream_t)stream, args...);
    return SMZ_OK;
}

// what every search launcher ends with: the tree is there for smz_root_stats / smz_act, no selection is pending
int search_launched(smz_handle *h) {
    h->root_ready = true;
    h->selected = false;
    return launch_check();
}

// dispatch on the per-lane scratch bucket (smallest MAXA >= A)
#define SMZ_DISPATCH(maxa, ...)               \
    switch (maxa) {                           \
        case 2: { constexpr int MA = 2; __VA_ARGS__; } break;   \
        case 4: { constexpr int MA = 4; __VA_ARGS__; } break;   \
        case 8: { constexpr int MA = 8; __VA_ARGS__; } break;   \
        case 16: { constexpr int MA = 16; __VA_ARGS__; } break; \
        default: { constexpr int MA = 32; __VA_ARGS__; } break; \
    }
// same, plus the exact-action-count specialisation for the two small buckets (aex: A == bucket)
#define SMZ_DISPATCH_AEX(maxa, aex, ...)                                                             \
    switch (maxa) {                                                                                  \
        case 2: if (aex) { constexpr int MA = 2; constexpr bool AEX = true; __VA_ARGS__; }            \
                else { constexpr int MA = 2; constexpr bool AEX = false; __VA_ARGS__; } break;        \
        case 4: if (aex) { constexpr int MA = 4; constexpr bool AEX = true; __VA_ARGS__; }            \
                else { constexpr int MA = 4; constexpr bool AEX = false; __VA_ARGS__; } break;        \
        case 8: { constexpr int MA = 8; constexpr bool AEX = false; __VA_ARGS__; } break;             \
        case 16: { constexpr int MA = 16; constexpr bool AEX = false; __VA_ARGS__; } break;           \
        default: { constexpr int MA = 32; constexpr bool AEX = false; __VA_ARGS__; } break;           \
    }
#define SMZ_DISPATCH2_AEX(maxa, k, aex, ...)                                          \
    if ((k) == 2) { constexpr int KS = 2; SMZ_DISPATCH_AEX(maxa, aex, __VA_ARGS__); }  \
    else { constexpr int KS = 0; SMZ_DISPATCH_AEX(maxa, aex, __VA_ARGS__); }
// ... and on the children-per-expansion specialisation (KS = 2: the static two-child code, 0: run-time count)
#define SMZ_DISPATCH2(maxa, k, ...)                                          \
    if ((k) == 2) { constexpr int KS = 2; SMZ_DISPATCH(maxa, __VA_ARGS__); }  \
    else { constexpr int KS = 0; SMZ_DISPATCH(maxa, __VA_ARGS__); }

}  // namespace

// the step-wise calls of a large-action handle (defined in smz_large_actions.hip)
int smz_internal_la_root_init(smz_handle *h, const float *hidden_dev, const float *policy_dev, const double *noise_override_dev,
                              int train, smz_stream stream);
int smz_internal_la_select(smz_handle *h, float *parent_hidden_dev, int32_t *last_action_dev, uint8_t *branch_dev,
                           float *mlp_input_dev, smz_stream stream);
int smz_internal_la_expand_backup(smz_handle *h, const float *hidden_dev, const float *reward_dev, const float *policy_dev,
                                  const float *value_dev, smz_stream stream);
int smz_internal_la_act(smz_handle *h, const Params &P, double temperature, int32_t *action_dev, double *policy_dev,
                        double *child_visits_dev, float *root_value_dev, smz_stream stream);
