// smz_env2048.hip -- the device-resident 2048 environment (C ABI: smz_2048_reset, smz_2048_step_ctl, smz_2048_host_step,
// smz_2048_host_reset).
//
// The first built-in env with chance in it: after every legal move a tile spawns (Stochastic MuZero's own single-player
// benchmark).  The rules live in smz_2048.hpp, one body for both sides; this unit adds the draws, the game bookkeeping of
// smz_episode_ctl (limit, mask / restart at a game's end, the reference's illegal-move rule, game.py:123-131) and the
// trajectory record, all in ONE launch per env step: one lane per env, the board in four registers.
//
// Draws: game_seed = reset_seed + (first_env + e) + 1000003 * episode (uint64 arithmetic: the seed host_envs.HostSlice hands
// to env.reset), and spawn number n of a game uses u_c = smz_unit(game_seed, 0, n, c), c = 0, 1 -- n = 0, 1 are the two tiles
// of the initial board, n = 2 + (legal moves made so far) the spawn after a move.  Nothing depends on the shard or on the
// launch geometry.
//
// Memory shape: per env and step 16 bytes of board in and out (one 128-bit access each way), 64 bytes of observation out
// (four 128-bit stores), a handful of scalars, and the 31 float64 of the record, which go out through LDS so that the
// wavefront's stores are contiguous (k_2048_step_env).
#include "smz_handle.hpp"
#include "smz_2048.hpp"

namespace {

constexpr int kObs = 16, kA = 4, kF = kObs + 3 * kA + 3;     // smz_traj_floats(16, 4) = 31

struct Env2048 {
    uint8_t *board;                // [B][16] u8 in/out
    int32_t *spawns;               // [B] i32 in/out: tiles spawned in the current game
    float *obs_out, *reward_out;
    uint8_t *flag_out;
    int32_t *step_count, *episode;
    uint8_t *active;
    int limit, on_end;
    uint64_t seed;
    long long first_env;
    double *traj;                  // [T][B][31] f64 or nullptr
    int t;
};

__host__ __device__ inline uint64_t game_seed_of(uint64_t seed, long long env, long long episode) {
    return seed + (uint64_t)env + 1000003ull * (uint64_t)episode;
}

__host__ __device__ inline void draw_spawn(uint32_t w[4], uint64_t game_seed, int n) {
    const double u0 = smz_unit(game_seed, 0, (uint64_t)n, 0), u1 = smz_unit(game_seed, 0, (uint64_t)n, 1);
    smz2048::spawn(w, u0, u1);
}

__host__ __device__ inline void initial_board(uint32_t w[4], uint64_t game_seed) {
    w[0] = w[1] = w[2] = w[3] = 0;
    draw_spawn(w, game_seed, 0);
    draw_spawn(w, game_seed, 1);
}

// One move of one game: the shared body of the kernel and of smz_2048_host_step.  Returns whether the move was legal; an
// illegal one (an action outside 0 .. 3 included) changes nothing.  `dead`: no action is legal on the board as it is now.
__host__ __device__ inline bool play_move(uint32_t w[4], int &spawns, int action, uint64_t game_seed, uint32_t &gain, bool &dead) {
    gain = 0;
    const bool legal = action >= 0 && action < kA && smz2048::move(w, action, gain);
    if (legal) {
        draw_spawn(w, game_seed, spawns);
        spawns++;
    }
    dead = !smz2048::any_legal(w);
    return legal;
}

// obs[i] = exponent[i] / 16, exact in float32
__device__ inline void write_obs(float *obs, const uint32_t w[4]) {
    float4 *o = reinterpret_cast<float4 *>(obs);
#pragma unroll
    for (int r = 0; r < 4; r++)
        o[r] = make_float4((float)(w[r] & 255u) * 0.0625f, (float)((w[r] >> 8) & 255u) * 0.0625f,
                           (float)((w[r] >> 16) & 255u) * 0.0625f, (float)(w[r] >> 24) * 0.0625f);
}

__global__ void __launch_bounds__(256) k_2048_reset(uint8_t *board, int32_t *spawns, float *obs_out, uint64_t seed,
                                                    long long first_env, const int32_t *episode, int B) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B) return;
    uint32_t w[4];
    initial_board(w, game_seed_of(seed, first_env + e, episode ? episode[e] : 0));
    reinterpret_cast<uint4 *>(board)[e] = make_uint4(w[0], w[1], w[2], w[3]);
    spawns[e] = 2;
    if (obs_out) write_obs(obs_out + (size_t)e * kObs, w);
}

// The step of env e with its game bookkeeping; r (nullptr: no record): where the 31 float64 of its record go.
__device__ inline void step_env(const Env2048 &E, int e, const int32_t *action, const double *policy, const double *child_visits,
                                const float *root_value, double *r) {
    if (E.active && !E.active[e]) {              // switched off: no step, the record says so
        if (E.flag_out) E.flag_out[e] = 3;
        if (E.reward_out) E.reward_out[e] = 0.f;
        if (r) { for (int k = 0; k < kF; k++) r[k] = 0.0; r[kObs + 1] = 3.0; }
        return;
    }
    const uint4 b = reinterpret_cast<const uint4 *>(E.board)[e];
    uint32_t w[4] = {b.x, b.y, b.z, b.w};
    int spawns = E.spawns[e];
    int ep = E.episode ? E.episode[e] : 0;
    const int before = E.step_count[e], act = action[e];
    uint32_t gain;
    bool dead;
    const bool legal = play_move(w, spawns, act, game_seed_of(E.seed, E.first_env + e, ep), gain, dead);
    const float reward = legal ? (float)gain : smz2048::illegal_reward(before, E.limit);
    int count = before + 1;                      // (an illegal move counts as a move, game.py:123-131)
    const int flag = (E.limit > 0 && count == E.limit) ? 2 : (dead ? 1 : 0);
    if (r) {
#pragma unroll
        for (int i = 0; i < kObs; i++) r[i] = (double)((float)((w[i >> 2] >> (8 * (i & 3))) & 255u) * 0.0625f);
        r[kObs] = (double)reward;
        r[kObs + 1] = (double)flag;
#pragma unroll
        for (int a = 0; a < kA; a++) {
            r[kObs + 2 + a] = policy[(size_t)e * kA + a];
            r[kObs + 2 + kA + a] = a == act ? 1.0 : 0.0;
            r[kObs + 3 + 2 * kA + a] = child_visits[(size_t)e * kA + a];
        }
        r[kObs + 2 + 2 * kA] = (double)root_value[e];
    }
    if (E.reward_out) E.reward_out[e] = reward;
    if (E.flag_out) E.flag_out[e] = (uint8_t)flag;
    if (flag != 0 && E.on_end == 2) {            // the record keeps the finished game's last board; the env starts its next game
        ep++;
        E.episode[e] = ep;
        initial_board(w, game_seed_of(E.seed, E.first_env + e, ep));
        spawns = 2;
        count = 0;
    } else if (flag != 0 && E.on_end == 1) {
        E.active[e] = 0;
    }
    E.step_count[e] = count;
    if (legal || (flag != 0 && E.on_end == 2)) {
        reinterpret_cast<uint4 *>(E.board)[e] = make_uint4(w[0], w[1], w[2], w[3]);
        E.spawns[e] = spawns;
        if (E.obs_out) write_obs(E.obs_out + (size_t)e * kObs, w);
    }
}

// One lane per env, one wavefront per workgroup (4096 envs: 64 workgroups, so the launch spreads over 64 compute units; the
// step is a chain of dependent loads and 64-bit integer arithmetic, latency not throughput).  The records of a workgroup's envs
// are one contiguous run of the step's slab: the lanes build their rows in LDS (16 KB) and the wavefront writes the run with
// coalesced 512-byte stores -- a lane writing its own row would touch 31 different cache lines, 248 bytes apart from its
// neighbour's.
constexpr int kStepThreads = 64;
__global__ void __launch_bounds__(kStepThreads) k_2048_step_env(Env2048 E, const int32_t *action, int B, const double *policy,
                                                                const double *child_visits, const float *root_value) {
    __shared__ double rows[kStepThreads * kF];
    const int e0 = blockIdx.x * kStepThreads, e = e0 + (int)threadIdx.x;
    if (e < B) step_env(E, e, action, policy, child_visits, root_value, E.traj ? rows + threadIdx.x * kF : nullptr);
    if (!E.traj) return;                         // (the same for every lane)
    __syncthreads();
    const int n = (B - e0 < kStepThreads ? B - e0 : kStepThreads) * kF;
    double *run = E.traj + ((size_t)E.t * B + e0) * kF;
    for (int i = threadIdx.x; i < n; i += kStepThreads) run[i] = rows[i];
}

inline bool misaligned16(const void *p) { return ((uintptr_t)p & 15u) != 0; }

}  // namespace

extern "C" {

int smz_2048_reset(uint8_t *board_dev, int32_t *spawns_dev, float *obs_out_dev, uint64_t seed, int64_t first_env,
                   const int32_t *episode_dev, int B, smz_stream stream) {
    if (!board_dev || !spawns_dev || B < 1) return fail(SMZ_ERR_INVALID, "smz_2048_reset: bad argument%s");
    if (misaligned16(board_dev) || misaligned16(obs_out_dev))
        return fail(SMZ_ERR_INVALID, "smz_2048_reset: board_dev and obs_out_dev must be 16-byte aligned%s");
    hipLaunchKernelGGL(k_2048_reset, row_grid(B), dim3(256), 0, (hipStream_t)stream, board_dev, spawns_dev, obs_out_dev, seed,
                       (long long)first_env, episode_dev, B);
    return launch_check();
}

int smz_2048_step_ctl(uint8_t *board_dev, int32_t *spawns_dev, const int32_t *action_dev, float *obs_out_dev,
                      float *reward_out_dev, uint8_t *flag_out_dev, const smz_episode_ctl *ctl, double *traj_dev, int T, int t,
                      const double *policy_dev, const double *child_visits_dev, const float *root_value_dev, int B,
                      smz_stream stream) {
    if (!board_dev || !spawns_dev || !action_dev || !ctl || !ctl->step_count_dev || B < 1)
        return fail(SMZ_ERR_INVALID, "smz_2048_step_ctl: bad argument%s");
    if (ctl->on_end < 0 || ctl->on_end > 2 || (ctl->on_end == 2 && !ctl->episode_dev) || (ctl->on_end == 1 && !ctl->active_dev))
        return fail(SMZ_ERR_INVALID, "smz_2048_step_ctl: on_end 1 needs active_dev, on_end 2 needs episode_dev%s");
    if (traj_dev && (!policy_dev || !child_visits_dev || !root_value_dev || t < 0 || t >= T))
        return fail(SMZ_ERR_INVALID, "smz_2048_step_ctl: bad trajectory argument%s");
    if (misaligned16(board_dev) || misaligned16(obs_out_dev))
        return fail(SMZ_ERR_INVALID, "smz_2048_step_ctl: board_dev and obs_out_dev must be 16-byte aligned%s");
    const Env2048 E = {board_dev, spawns_dev, obs_out_dev, reward_out_dev, flag_out_dev, ctl->step_count_dev, ctl->episode_dev,
                       ctl->active_dev, ctl->limit, ctl->on_end, (uint64_t)ctl->reset_seed, (long long)ctl->first_env, traj_dev, t};
    hipLaunchKernelGGL(k_2048_step_env, dim3((unsigned)((B + kStepThreads - 1) / kStepThreads)), dim3(kStepThreads), 0,
                       (hipStream_t)stream, E, action_dev, B, policy_dev, child_visits_dev, root_value_dev);
    return launch_check();
}

int smz_2048_host_reset(uint8_t board[16], int32_t *spawns, uint64_t game_seed) {
    if (!board || !spawns) return fail(SMZ_ERR_INVALID, "smz_2048_host_reset: null argument%s");
    uint32_t w[4];
    initial_board(w, game_seed);
    smz2048::store(w, board);
    *spawns = 2;
    return SMZ_OK;
}

int smz_2048_host_step(uint8_t board[16], int32_t *spawns, int action, uint64_t game_seed, float *reward_out,
                       int *terminated_out, int *illegal_out) {
    if (!board || !spawns) return fail(SMZ_ERR_INVALID, "smz_2048_host_step: null argument%s");
    uint32_t w[4], gain;
    smz2048::load(board, w);
    int n = *spawns;
    bool dead;
    const bool legal = play_move(w, n, action, game_seed, gain, dead);
    if (legal) {
        smz2048::store(w, board);
        *spawns = n;
    }
    if (reward_out) *reward_out = legal ? (float)gain : 0.f;
    if (terminated_out) *terminated_out = dead ? 1 : 0;
    if (illegal_out) *illegal_out = legal ? 0 : 1;
    return SMZ_OK;
}

}  // extern "C"
