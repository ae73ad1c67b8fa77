// smz_env_frame.hpp -- what the device-resident board games share (smz_env2048.hip, smz_envconnect4.hip, smz_envothello.hip): the game bookkeeping
// of smz_episode_ctl (limit, mask / restart at a game's end, the reference's illegal-move rule, game.py:123-131), the trajectory
// record, the step kernel and the argument checks of the *_step_ctl entry points.  A game brings its rules as a traits struct:
//
//   struct Game {                                      // passed to the kernel by value: it holds the game's state pointers
//       static constexpr int kObs, kA;                 // observations and actions of one env
//       struct State;                                  // one env's game in registers
//       __device__ State load(int e) const;            // the state of env e, with 128-bit accesses
//       __device__ void store(int e, const State &) const;
//       static bool play(State &, int action, uint64_t seed, long long env, long long episode, float &reward, bool &over);
//                                                      // one move; -> legal (an illegal move changes nothing, its reward
//                                                      // is not read); over: no move can follow on the state as it is now
//       static void restart(State &, uint64_t seed, long long env, long long episode);      // the first state of a game
//       template <typename T> static void write_obs(T *row, const State &);                 // kObs values, float or double
//       static constexpr bool kStageObs;               // the observation rows go out through LDS (put_obs); false: the game
//       static void write_obs_direct(float *row, const State &);                            // ... stores its row in global memory
//       static constexpr int kEnvs;                    // OPTIONAL: the envs one 64-lane workgroup plays, a divisor of 64 (64
//                                                      // when absent).  A game with wide rows states fewer, so that its rows
//                                                      // fit LDS several workgroups to a compute unit (smz_envothello.hip)
//   };
//
// seed, env (the global index) and episode name the game for the draws of a game with chance; a game without ignores them.
#pragma once
#include "smz_handle.hpp"

namespace {

// The reward of an illegal move (game.py:123-131): min(-(steps so far), -limit, -1), -limit = -inf without a limit.
__host__ __device__ inline float illegal_reward(int steps_so_far, int limit) {
    float r = -(float)steps_so_far;
    const float l = limit > 0 ? -(float)limit : -INFINITY;
    if (l < r) r = l;
    if (-1.0f < r) r = -1.0f;
    return r;
}

struct EnvFrame {                  // the arguments of a step that do not depend on the game
    float *obs_out, *reward_out;
    uint8_t *flag_out;
    int32_t *step_count, *episode;
    uint8_t *active;
    int limit, on_end;
    uint64_t seed;
    long long first_env;
    double *traj;                  // [T][B][kObs + 3 kA + 3] f64 or nullptr
    int t;
};

// The observation of env e after its step; `changed`: the step stored a new state.  A game with kStageObs gets its LDS row `o`
// written whatever happened (a pure function of the state); one without writes the row in `obs_out` from its own lane, and only
// when it changed (2048: 64 bytes, four 128-bit stores; staged, its step missed the parent kernel's time by more than the
// parent's spread in both sessions that measured it: profiles/r21_env_frame_rate.txt).
template <class Game>
__device__ inline void put_obs(const EnvFrame &E, int e, float *o, const typename Game::State &s, bool changed) {
    if constexpr (Game::kStageObs) Game::write_obs(o, s);
    else if (changed && E.obs_out) Game::write_obs_direct(E.obs_out + (size_t)e * Game::kObs, s);
}

// The step of env e with its game bookkeeping.  r (nullptr: no record): the LDS row of its record, policy and child visits
// already in place; o: the LDS row of its observation (put_obs).
template <class Game>
__device__ inline void env_step_lane(const Game &G, const EnvFrame &E, int e, const int32_t *action, const float *root_value,
                                     double *r, float *o) {
    constexpr int kObs = Game::kObs, kA = Game::kA, kF = kObs + 3 * kA + 3;
    typename Game::State s = G.load(e);
    if (E.active && !E.active[e]) {              // switched off: no step, the record says so
        if (E.flag_out) E.flag_out[e] = 3;
        if (E.reward_out) E.reward_out[e] = 0.f;
        if (r) {
#pragma unroll
            for (int k = 0; k < kF; k++) r[k] = 0.0;
            r[kObs + 1] = 3.0;
        }
        put_obs<Game>(E, e, o, s, false);
        return;
    }
    int ep = E.episode ? E.episode[e] : 0;
    const int before = E.step_count[e], act = action[e];
    float reward;
    bool over;
    const bool legal = Game::play(s, act, E.seed, E.first_env + e, ep, reward, over);
    if (!legal) reward = illegal_reward(before, E.limit);
    int count = before + 1;                      // (an illegal move counts as a move, game.py:123-131)
    const int flag = (E.limit > 0 && count == E.limit) ? 2 : (over ? 1 : 0);
    if (r) {
        Game::write_obs(r, s);
        r[kObs] = (double)reward;
        r[kObs + 1] = (double)flag;
#pragma unroll
        for (int a = 0; a < kA; a++) r[kObs + 2 + kA + a] = a == act ? 1.0 : 0.0;
        r[kObs + 2 + 2 * kA] = (double)root_value[e];
    }
    if (E.reward_out) E.reward_out[e] = reward;
    if (E.flag_out) E.flag_out[e] = (uint8_t)flag;
    const bool restart = flag != 0 && E.on_end == 2;
    if (restart) {                               // the record keeps the finished game's last state; the env starts its next game
        ep++;
        E.episode[e] = ep;
        Game::restart(s, E.seed, E.first_env + e, ep);
        count = 0;
    } else if (flag != 0 && E.on_end == 1) {
        E.active[e] = 0;
    }
    E.step_count[e] = count;
    if (legal || restart) G.store(e, s);
    put_obs<Game>(E, e, o, s, legal || restart);
}

// The envs of one workgroup: Game::kEnvs where the game states it, else one per lane.
template <class Game, class = void>
struct EnvsPerGroup {
    static constexpr int value = 64;
};
template <class Game>
struct EnvsPerGroup<Game, decltype((void)Game::kEnvs)> {
    static constexpr int value = Game::kEnvs;
};

// One lane per env, one wavefront per workgroup (4096 envs: 64 workgroups, so the launch spreads over 64 compute units; the
// step is a short chain of dependent loads and integer arithmetic, latency not throughput).  The record rows (kF float64) and,
// with kStageObs, the observation rows (kObs float32) of a workgroup's envs are one contiguous run each, built in LDS and
// written out with coalesced stores: 64 x 8 kF bytes = 15.5 KB for 2048, 64 x (4 kObs + 8 kF) = 44.25 KB for Connect Four.  A
// lane writing its own rows would touch cache lines that its neighbours touch again.  The policy and child-visit rows come in
// the same way: [n][kA] float64 is contiguous per workgroup, read coalesced and scattered into the LDS rows.
// A game with kEnvs < 64 has lanes < kEnvs play; all 64 lanes move the runs, and LDS holds kEnvs rows (Othello: 16 x 2364 bytes
// = 36.9 KB and 256 workgroups for 4096 envs; with 64 envs per workgroup its 147.75 KB leave one workgroup to a compute unit and
// the launch takes twice as long, profiles/r22_othello_rate.txt).
constexpr int kStepThreads = 64;
template <class Game>
__global__ void __launch_bounds__(kStepThreads) k_board_step_env(Game G, EnvFrame E, const int32_t *action, int B,
                                                                 const double *policy, const double *child_visits,
                                                                 const float *root_value) {
    constexpr int kObs = Game::kObs, kA = Game::kA, kF = kObs + 3 * kA + 3, kEnvs = EnvsPerGroup<Game>::value;
    static_assert(kEnvs >= 1 && kEnvs <= kStepThreads && kStepThreads % kEnvs == 0, "kEnvs divides the workgroup");
    __shared__ double rows[kEnvs * kF];
    float *obs_rows = nullptr;
    if constexpr (Game::kStageObs) {
        __shared__ float staged[kEnvs * kObs];
        obs_rows = staged;
    }
    const int lane = (int)threadIdx.x, e0 = blockIdx.x * kEnvs, e = e0 + lane;
    const int n = B - e0 < kEnvs ? B - e0 : kEnvs;                       // envs of this workgroup (>= 1 by the grid)
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
    if (kEnvs == kStepThreads ? e < B : lane < n) env_step_lane(G, E, e, action, root_value, record ? rows + lane * kF : nullptr,
                               Game::kStageObs ? obs_rows + lane * kObs : nullptr);
    __syncthreads();
    if (Game::kStageObs && E.obs_out) {
        float *run = E.obs_out + (size_t)e0 * kObs;
        for (int i = lane; i < n * kObs; i += kStepThreads) run[i] = obs_rows[i];
    }
    if (record) {
        double *run = E.traj + ((size_t)E.t * B + e0) * kF;
        for (int i = lane; i < n * kF; i += kStepThreads) run[i] = rows[i];
    }
}

inline bool misaligned16(const void *p) { return ((uintptr_t)p & 15u) != 0; }

// What every *_step_ctl entry point requires of its smz_episode_ctl and its trajectory arguments; the refusal is in the
// last-error text.
bool env_step_args_ok(const char *name, const smz_episode_ctl *ctl, const double *traj, const double *policy,
                      const double *child_visits, const float *root_value, int T, int t) {
    if (!ctl) return fail(SMZ_ERR_INVALID, "%s: bad argument", name), false;
    if (!episode_ctl_ok(name, ctl)) return false;
    if (traj && (!policy || !child_visits || !root_value || t < 0 || t >= T))
        return fail(SMZ_ERR_INVALID, "%s: bad trajectory argument", name), false;
    return true;
}

// The launch of a board game's step: G holds the state pointers, the rest comes from the entry point's arguments as checked.
template <class Game>
int launch_board_step(const Game &G, const int32_t *action_dev, float *obs_out_dev, float *reward_out_dev, uint8_t *flag_out_dev,
                      const smz_episode_ctl *ctl, double *traj_dev, int t, const double *policy_dev,
                      const double *child_visits_dev, const float *root_value_dev, int B, smz_stream stream) {
    const EnvFrame E = {obs_out_dev, reward_out_dev, flag_out_dev, ctl->step_count_dev, ctl->episode_dev, ctl->active_dev,
                        ctl->limit, ctl->on_end, (uint64_t)ctl->reset_seed, (long long)ctl->first_env, traj_dev, t};
    constexpr int kEnvs = EnvsPerGroup<Game>::value;
    hipLaunchKernelGGL(k_board_step_env<Game>, dim3((unsigned)((B + kEnvs - 1) / kEnvs)), dim3(kStepThreads), 0,
                       (hipStream_t)stream, G, E, action_dev, B, policy_dev, child_visits_dev, root_value_dev);
    return launch_check();
}

}  // namespace
