// smz_env2048.hip -- the device-resident 2048 environment (C ABI: smz_2048_reset, smz_2048_step_ctl, smz_2048_host_step,
// smz_2048_host_reset).
//
// The first built-in env with chance in it: after every legal move a tile spawns (Stochastic MuZero's own single-player
// benchmark).  The rules live in smz_2048.hpp, one body for both sides; this unit adds the draws and states the game to
// smz_env_frame.hpp (Game2048), which holds the game bookkeeping, the trajectory record and the step kernel: ONE launch per env
// step, one lane per env, the board in four registers.
//
// Draws: game_seed = reset_seed + (first_env + e) + 1000003 * episode (uint64 arithmetic: the seed host_envs.HostSlice hands
// to env.reset), and spawn number n of a game uses u_c = smz_unit(game_seed, 0, n, c), c = 0, 1 -- n = 0, 1 are the two tiles
// of the initial board, n = 2 + (legal moves made so far) the spawn after a move.  Nothing depends on the shard or on the
// launch geometry.
//
// Memory shape: per env and step 16 bytes of board in and out (one 128-bit access each way), 64 bytes of observation out
// (four 128-bit stores), a handful of scalars, and the 31 float64 of the record, which go out through LDS (k_board_step_env).
#include "smz_env_frame.hpp"
#include "smz_2048.hpp"

namespace {

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
    const bool legal = action >= 0 && action < 4 && smz2048::move(w, action, gain);
    if (legal) {
        draw_spawn(w, game_seed, spawns);
        spawns++;
    }
    dead = !smz2048::any_legal(w);
    return legal;
}

struct Game2048 {
    static constexpr int kObs = 16, kA = 4;      // smz_traj_floats(16, 4) = 31
    uint8_t *board;                // [B][16] u8 in/out
    int32_t *spawns;               // [B] i32 in/out: tiles spawned in the current game
    struct State {
        uint32_t w[4];             // the rows (smz_2048.hpp)
        int spawns;
    };
    __device__ State load(int e) const {
        const uint4 b = reinterpret_cast<const uint4 *>(board)[e];
        return {{b.x, b.y, b.z, b.w}, spawns[e]};
    }
    __device__ void store(int e, const State &s) const {
        reinterpret_cast<uint4 *>(board)[e] = make_uint4(s.w[0], s.w[1], s.w[2], s.w[3]);
        spawns[e] = s.spawns;
    }
    __device__ static bool play(State &s, int action, uint64_t seed, long long env, long long episode, float &reward, bool &over) {
        uint32_t gain;
        const bool legal = play_move(s.w, s.spawns, action, game_seed_of(seed, env, episode), gain, over);
        reward = (float)gain;
        return legal;
    }
    __device__ static void restart(State &s, uint64_t seed, long long env, long long episode) {
        initial_board(s.w, game_seed_of(seed, env, episode));
        s.spawns = 2;
    }
    // obs[i] = exponent[i] / 16, exact in float32
    template <typename T>
    __device__ static void write_obs(T *row, const State &s) {
#pragma unroll
        for (int i = 0; i < kObs; i++) row[i] = (T)((float)((s.w[i >> 2] >> (8 * (i & 3))) & 255u) * 0.0625f);
    }
    // The row in global memory (16-byte aligned) is four 128-bit stores of the env's own lane, not staged in LDS.
    static constexpr bool kStageObs = false;
    __device__ static void write_obs_direct(float *row, const State &s) {
        float o[kObs];
        write_obs(o, s);
#pragma unroll
        for (int r = 0; r < 4; r++) reinterpret_cast<float4 *>(row)[r] = make_float4(o[4 * r], o[4 * r + 1], o[4 * r + 2], o[4 * r + 3]);
    }
};

__global__ void __launch_bounds__(256) k_2048_reset(uint8_t *board, int32_t *spawns, float *obs_out, uint64_t seed,
                                                    long long first_env, const int32_t *episode, int B) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B) return;
    Game2048::State s;
    Game2048::restart(s, seed, first_env + e, episode ? episode[e] : 0);
    Game2048{board, spawns}.store(e, s);
    if (obs_out) Game2048::write_obs_direct(obs_out + (size_t)e * Game2048::kObs, s);
}

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
    if (!board_dev || !spawns_dev || !action_dev || B < 1) return fail(SMZ_ERR_INVALID, "smz_2048_step_ctl: bad argument%s");
    if (!env_step_args_ok("smz_2048_step_ctl", ctl, traj_dev, policy_dev, child_visits_dev, root_value_dev, T, t))
        return SMZ_ERR_INVALID;
    if (misaligned16(board_dev) || misaligned16(obs_out_dev))
        return fail(SMZ_ERR_INVALID, "smz_2048_step_ctl: board_dev and obs_out_dev must be 16-byte aligned%s");
    return launch_board_step(Game2048{board_dev, spawns_dev}, action_dev, obs_out_dev, reward_out_dev, flag_out_dev, ctl, traj_dev,
                             t, policy_dev, child_visits_dev, root_value_dev, B, stream);
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
