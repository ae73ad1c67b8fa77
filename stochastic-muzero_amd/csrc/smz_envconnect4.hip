// smz_envconnect4.hip -- the device-resident Connect Four environment (C ABI: smz_connect4_reset, smz_connect4_step_ctl,
// smz_connect4_host_step).
//
// The built-in env with TWO players: the colours move in turn and the side to move is read off the board.  The rules live in
// smz_connect4.hpp, one body for both sides; this unit states the game to smz_env_frame.hpp (GameConnect4), which holds the
// game bookkeeping, the trajectory record and the step kernel: ONE launch per env step, one lane per env, the position in two
// 64-bit registers.  The game is deterministic: nothing is drawn.
//
// Memory shape: per env and step 16 bytes of position in and out (one 128-bit access each way), the 172 bytes of its
// observation row and the 536 bytes of its record row, which go out through LDS (k_board_step_env).
#include "smz_env_frame.hpp"
#include "smz_connect4.hpp"

namespace {

struct GameConnect4 {
    static constexpr int kObs = 43, kA = 7;      // smz_traj_floats(43, 7) = 67
    static constexpr bool kStageObs = true;      // (172 bytes a row: written by its lane it would touch 3 cache lines)
    uint64_t *discs;               // [B][2] u64 in/out
    struct State {
        uint64_t d0, d1;           // the discs of colour 0 and of colour 1 (smz_connect4.hpp)
    };
    __device__ State load(int e) const {
        const ulonglong2 b = reinterpret_cast<const ulonglong2 *>(discs)[e];
        return {b.x, b.y};
    }
    __device__ void store(int e, const State &s) const { reinterpret_cast<ulonglong2 *>(discs)[e] = make_ulonglong2(s.d0, s.d1); }
    __device__ static bool play(State &s, int action, uint64_t, long long, long long, float &reward, bool &over) {
        bool won;
        const bool legal = smzc4::play(s.d0, s.d1, action, won, over);
        reward = won ? 1.0f : 0.0f;
        return legal;
    }
    __device__ static void restart(State &s, uint64_t, long long, long long) { s.d0 = s.d1 = 0; }
    // (every index is a compile-time constant)
    template <typename T>
    __device__ static void write_obs(T *row, const State &s) {
#pragma unroll
        for (int r = 0; r < smzc4::kRows; r++)
#pragma unroll
            for (int c = 0; c < smzc4::kCols; c++) row[7 * r + c] = (T)smzc4::cell_obs(s.d0, s.d1, r, c);
        row[kObs - 1] = (T)smzc4::mover_obs(s.d0, s.d1);
    }
};

__global__ void __launch_bounds__(256) k_connect4_reset(uint64_t *discs, float *obs_out, int B) {
    constexpr int kObs = GameConnect4::kObs;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) reinterpret_cast<ulonglong2 *>(discs)[i] = make_ulonglong2(0ull, 0ull);
    if (obs_out && i < (long long)B * kObs) obs_out[i] = (i % kObs == kObs - 1) ? 1.0f : 0.0f;     // empty, colour 0 to move
}

}  // namespace

extern "C" {

int smz_connect4_reset(uint64_t *discs_dev, float *obs_out_dev, int B, smz_stream stream) {
    if (!discs_dev || B < 1) return fail(SMZ_ERR_INVALID, "smz_connect4_reset: bad argument%s");
    if (misaligned16(discs_dev)) return fail(SMZ_ERR_INVALID, "smz_connect4_reset: discs_dev must be 16-byte aligned%s");
    const long long items = (long long)B * GameConnect4::kObs;
    hipLaunchKernelGGL(k_connect4_reset, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, discs_dev,
                       obs_out_dev, B);
    return launch_check();
}

int smz_connect4_step_ctl(uint64_t *discs_dev, const int32_t *action_dev, float *obs_out_dev, float *reward_out_dev,
                          uint8_t *flag_out_dev, const smz_episode_ctl *ctl, double *traj_dev, int T, int t,
                          const double *policy_dev, const double *child_visits_dev, const float *root_value_dev, int B,
                          smz_stream stream) {
    if (!discs_dev || !action_dev || B < 1) return fail(SMZ_ERR_INVALID, "smz_connect4_step_ctl: bad argument%s");
    if (!env_step_args_ok("smz_connect4_step_ctl", ctl, traj_dev, policy_dev, child_visits_dev, root_value_dev, T, t))
        return SMZ_ERR_INVALID;
    if (misaligned16(discs_dev)) return fail(SMZ_ERR_INVALID, "smz_connect4_step_ctl: discs_dev must be 16-byte aligned%s");
    return launch_board_step(GameConnect4{discs_dev}, action_dev, obs_out_dev, reward_out_dev, flag_out_dev, ctl, traj_dev, t,
                             policy_dev, child_visits_dev, root_value_dev, B, stream);
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
