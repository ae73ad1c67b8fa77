// smz_envconnect4.hip -- the device-resident Connect Four environment (C ABI: smz_connect4_reset, smz_connect4_step_ctl,
// smz_connect4_host_step).
//
// The built-in env with TWO players: the colours move in turn and the side to move is read off the board.  The rules live in
// smz_connect4.hpp, one body for both sides; this unit adds the game bookkeeping of smz_episode_ctl (limit, mask / restart at a
// game's end, the reference's illegal-move rule, game.py:123-131) and the trajectory record, all in ONE launch per env step:
// one lane per env, the position in two 64-bit registers.  The game is deterministic: nothing is drawn.
//
// Memory shape: per env and step 16 bytes of position in and out (one 128-bit access each way), the 172 bytes of its
// observation row and the 536 bytes of its record row.  Neither row is written by its lane: a workgroup's rows are contiguous in
// both arrays, so the lanes build them in LDS and the wavefront writes each run with coalesced stores (k_connect4_step_env).
#include "smz_handle.hpp"
#include "smz_connect4.hpp"

namespace {

constexpr int kObs = 43, kA = 7, kF = kObs + 3 * kA + 3;     // smz_traj_floats(43, 7) = 67

struct EnvConnect4 {
    uint64_t *discs;               // [B][2] u64 in/out
    float *obs_out, *reward_out;
    uint8_t *flag_out;
    int32_t *step_count, *episode;
    uint8_t *active;
    int limit, on_end;
    double *traj;                  // [T][B][67] f64 or nullptr
    int t;
};

// The observation of a position into row `o` (float or double; LDS): every index is a compile-time constant.
template <typename T>
__device__ inline void write_obs(T *o, uint64_t d0, uint64_t d1) {
#pragma unroll
    for (int r = 0; r < smzc4::kRows; r++)
#pragma unroll
        for (int c = 0; c < smzc4::kCols; c++) o[7 * r + c] = (T)smzc4::cell_obs(d0, d1, r, c);
    o[kObs - 1] = (T)smzc4::mover_obs(d0, d1);
}

__global__ void __launch_bounds__(256) k_connect4_reset(uint64_t *discs, float *obs_out, int B) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) reinterpret_cast<ulonglong2 *>(discs)[i] = make_ulonglong2(0ull, 0ull);
    if (obs_out && i < (long long)B * kObs) obs_out[i] = (i % kObs == kObs - 1) ? 1.0f : 0.0f;     // empty, colour 0 to move
}

// The step of env e with its game bookkeeping.  r (nullptr: no record): the LDS row of its record, policy and child visits
// already in place; o: the LDS row of its observation, always written (a pure function of the position).
__device__ inline void step_env(const EnvConnect4 &E, int e, const int32_t *action, const float *root_value, double *r, float *o) {
    const ulonglong2 b = reinterpret_cast<const ulonglong2 *>(E.discs)[e];
    uint64_t d0 = b.x, d1 = b.y;
    if (E.active && !E.active[e]) {              // switched off: no step, the record says so
        if (E.flag_out) E.flag_out[e] = 3;
        if (E.reward_out) E.reward_out[e] = 0.f;
        if (r) {
#pragma unroll
            for (int k = 0; k < kF; k++) r[k] = 0.0;
            r[kObs + 1] = 3.0;
        }
        write_obs(o, d0, d1);
        return;
    }
    const int before = E.step_count[e], act = action[e];
    bool won, over;
    const bool legal = smzc4::play(d0, d1, act, won, over);
    const float reward = legal ? (won ? 1.0f : 0.0f) : smzc4::illegal_reward(before, E.limit);
    int count = before + 1;                      // (an illegal move counts as a move, game.py:123-131)
    const int flag = (E.limit > 0 && count == E.limit) ? 2 : (over ? 1 : 0);
    if (r) {
        write_obs(r, d0, d1);
        r[kObs] = (double)reward;
        r[kObs + 1] = (double)flag;
#pragma unroll
        for (int a = 0; a < kA; a++) r[kObs + 2 + kA + a] = a == act ? 1.0 : 0.0;
        r[kObs + 2 + 2 * kA] = (double)root_value[e];
    }
    if (E.reward_out) E.reward_out[e] = reward;
    if (E.flag_out) E.flag_out[e] = (uint8_t)flag;
    const bool restart = flag != 0 && E.on_end == 2;
    if (restart) {                               // the record keeps the finished game's last board; the env starts its next game
        E.episode[e] += 1;
        d0 = d1 = 0;
        count = 0;
    } else if (flag != 0 && E.on_end == 1) {
        E.active[e] = 0;
    }
    E.step_count[e] = count;
    if (legal || restart) reinterpret_cast<ulonglong2 *>(E.discs)[e] = make_ulonglong2(d0, d1);
    write_obs(o, d0, d1);
}

// One lane per env, one wavefront per workgroup (4096 envs: 64 workgroups; the step is a short chain of dependent loads and
// 64-bit integer arithmetic, latency not throughput).  The observation rows (43 float32) and the record rows (67 float64) of a
// workgroup's envs are one contiguous run each: 64 x 172 + 64 x 536 bytes = 44.25 KB of LDS, written out with coalesced stores.
// A lane writing its own rows would touch 3 + 9 cache lines that its neighbours touch again.  The policy and child-visit rows
// come in the same way: [n][7] float64 is contiguous per workgroup, read coalesced and scattered into the LDS rows.
constexpr int kStepThreads = 64;
__global__ void __launch_bounds__(kStepThreads) k_connect4_step_env(EnvConnect4 E, const int32_t *action, int B, const double *policy,
                                                                    const double *child_visits, const float *root_value) {
    __shared__ double rows[kStepThreads * kF];
    __shared__ float obs_rows[kStepThreads * kObs];
    const int lane = (int)threadIdx.x, e0 = blockIdx.x * kStepThreads, e = e0 + lane;
    const int n = B - e0 < kStepThreads ? B - e0 : kStepThreads;         // envs of this workgroup (>= 1 by the grid)
    const bool record = E.traj != nullptr;                               // (the same for every lane)
    if (record) {
        const double *p = policy + (size_t)e0 * kA, *v = child_visits + (size_t)e0 * kA;
        for (int i = lane; i < n * kA; i += kStepThreads) {
            const int row = i / kA, a = i - row * kA;
            rows[row * kF + kObs + 2 + a] = p[i];
            rows[row * kF + kObs + 3 + 2 * kA + a] = v[i];
        }
        __syncthreads();                         // a switched-off env zeroes its whole row
    }
    if (e < B) step_env(E, e, action, root_value, record ? rows + lane * kF : nullptr, obs_rows + lane * kObs);
    __syncthreads();
    if (E.obs_out) {
        float *run = E.obs_out + (size_t)e0 * kObs;
        for (int i = lane; i < n * kObs; i += kStepThreads) run[i] = obs_rows[i];
    }
    if (record) {
        double *run = E.traj + ((size_t)E.t * B + e0) * kF;
        for (int i = lane; i < n * kF; i += kStepThreads) run[i] = rows[i];
    }
}

inline bool misaligned16(const void *p) { return ((uintptr_t)p & 15u) != 0; }

}  // namespace

extern "C" {

int smz_connect4_reset(uint64_t *discs_dev, float *obs_out_dev, int B, smz_stream stream) {
    if (!discs_dev || B < 1) return fail(SMZ_ERR_INVALID, "smz_connect4_reset: bad argument%s");
    if (misaligned16(discs_dev)) return fail(SMZ_ERR_INVALID, "smz_connect4_reset: discs_dev must be 16-byte aligned%s");
    const long long items = (long long)B * kObs;
    hipLaunchKernelGGL(k_connect4_reset, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, discs_dev,
                       obs_out_dev, B);
    return launch_check();
}

int smz_connect4_step_ctl(uint64_t *discs_dev, const int32_t *action_dev, float *obs_out_dev, float *reward_out_dev,
                          uint8_t *flag_out_dev, const smz_episode_ctl *ctl, double *traj_dev, int T, int t,
                          const double *policy_dev, const double *child_visits_dev, const float *root_value_dev, int B,
                          smz_stream stream) {
    if (!discs_dev || !action_dev || !ctl || !ctl->step_count_dev || B < 1)
        return fail(SMZ_ERR_INVALID, "smz_connect4_step_ctl: bad argument%s");
    if (ctl->on_end < 0 || ctl->on_end > 2 || (ctl->on_end == 2 && !ctl->episode_dev) || (ctl->on_end == 1 && !ctl->active_dev))
        return fail(SMZ_ERR_INVALID, "smz_connect4_step_ctl: on_end 1 needs active_dev, on_end 2 needs episode_dev%s");
    if (traj_dev && (!policy_dev || !child_visits_dev || !root_value_dev || t < 0 || t >= T))
        return fail(SMZ_ERR_INVALID, "smz_connect4_step_ctl: bad trajectory argument%s");
    if (misaligned16(discs_dev)) return fail(SMZ_ERR_INVALID, "smz_connect4_step_ctl: discs_dev must be 16-byte aligned%s");
    const EnvConnect4 E = {discs_dev, obs_out_dev, reward_out_dev, flag_out_dev, ctl->step_count_dev, ctl->episode_dev,
                           ctl->active_dev, ctl->limit, ctl->on_end, traj_dev, t};
    hipLaunchKernelGGL(k_connect4_step_env, dim3((unsigned)((B + kStepThreads - 1) / kStepThreads)), dim3(kStepThreads), 0,
                       (hipStream_t)stream, E, action_dev, B, policy_dev, child_visits_dev, root_value_dev);
    return launch_check();
}

int smz_connect4_host_step(uint64_t discs[2], int action, float *reward_out, int *terminated_out, int *illegal_out) {
    if (!discs) return fail(SMZ_ERR_INVALID, "smz_connect4_host_step: null argument%s");
    uint64_t d0 = discs[0], d1 = discs[1];
    bool won, over;
    const bool legal = smzc4::play(d0, d1, action, won, over);
    if (legal) {
        discs[0] = d0;
        discs[1] = d1;
    }
    if (reward_out) *reward_out = won ? 1.0f : 0.f;
    if (terminated_out) *terminated_out = over ? 1 : 0;
    if (illegal_out) *illegal_out = legal ? 0 : 1;
    return SMZ_OK;
}

}  // extern "C"
