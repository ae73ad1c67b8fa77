// smz_envothello.hip -- the device-resident Othello environment (C ABI: smz_othello_reset, smz_othello_step_ctl,
// smz_othello_host_step, smz_othello_host_moves).
//
// The built-in env with MORE THAN 32 actions: 64 squares and a pass, two colours, so a large-action handle
// (smz_create_large_actions) gets a real game.  The rules live in smz_othello.hpp, one body for both sides; this unit states
// the game to smz_env_frame.hpp (GameOthello), which holds the game bookkeeping, the trajectory record and the step kernel:
// ONE launch per env step, one lane per env, the position in two 64-bit registers and the colour to move in a third.  The game
// is deterministic: nothing is drawn.
//
// Memory shape: per env and step 16 bytes of position (one 128-bit access each way) and 4 bytes of mover in and out, the 260
// bytes of its observation row and the 2 104 bytes of its record row (smz_traj_floats(65, 65) = 263 float64), which go out
// through LDS (k_board_step_env).  A row pair is 2 364 bytes, so the frame's 64 envs per workgroup would take 151 296 bytes of
// LDS, one workgroup to a compute unit; kEnvs below is the measured choice.
#include "smz_env_frame.hpp"
#include "smz_othello.hpp"

#ifndef SMZ_OTHELLO_ENVS
#define SMZ_OTHELLO_ENVS 16
#endif

namespace {

struct GameOthello {
    static constexpr int kObs = 65, kA = 65;     // smz_traj_floats(65, 65) = 263
    static constexpr bool kStageObs = true;      // (260 bytes a row: written by its lane it would touch 5 cache lines)
    static constexpr int kEnvs = SMZ_OTHELLO_ENVS;             // envs per workgroup: kEnvs x 2 364 bytes of LDS
    uint64_t *discs;               // [B][2] u64 in/out
    int32_t *mover;                // [B] in/out
    struct State {
        uint64_t d0, d1;           // the discs of colour 0 and of colour 1 (smz_othello.hpp)
        int mover;                 // the colour to move
    };
    __device__ State load(int e) const {
        const ulonglong2 b = reinterpret_cast<const ulonglong2 *>(discs)[e];
        return {b.x, b.y, mover[e] != 0 ? 1 : 0};
    }
    __device__ void store(int e, const State &s) const {
        reinterpret_cast<ulonglong2 *>(discs)[e] = make_ulonglong2(s.d0, s.d1);
        mover[e] = s.mover;
    }
    __device__ static bool play(State &s, int action, uint64_t, long long, long long, float &reward, bool &over) {
        return smzoth::play(s.d0, s.d1, s.mover, action, reward, over);
    }
    __device__ static void restart(State &s, uint64_t, long long, long long) {
        s.d0 = smzoth::kStart0;
        s.d1 = smzoth::kStart1;
        s.mover = 0;
    }
    // (every index is a compile-time constant)
    template <typename T>
    __device__ static void write_obs(T *row, const State &s) {
        smzoth::write_obs(row, s.d0, s.d1, s.mover);
    }
};

__global__ void __launch_bounds__(256) k_othello_reset(uint64_t *discs, int32_t *mover, float *obs_out, int B) {
    constexpr int kObs = GameOthello::kObs;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) {
        reinterpret_cast<ulonglong2 *>(discs)[i] = make_ulonglong2(smzoth::kStart0, smzoth::kStart1);
        mover[i] = 0;
    }
    if (obs_out && i < (long long)B * kObs) {
        const int k = (int)(i % kObs);                        // the four centre squares, colour 0 to move
        obs_out[i] = (k == 28 || k == 35 || k == kObs - 1) ? 1.0f : ((k == 27 || k == 36) ? -1.0f : 0.0f);
    }
}

}  // namespace

extern "C" {

int smz_othello_reset(uint64_t *discs_dev, int32_t *mover_dev, float *obs_out_dev, int B, smz_stream stream) {
    if (!discs_dev || !mover_dev || B < 1) return fail(SMZ_ERR_INVALID, "smz_othello_reset: bad argument%s");
    if (misaligned16(discs_dev)) return fail(SMZ_ERR_INVALID, "smz_othello_reset: discs_dev must be 16-byte aligned%s");
    const long long items = (long long)B * GameOthello::kObs;
    hipLaunchKernelGGL(k_othello_reset, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, discs_dev,
                       mover_dev, obs_out_dev, B);
    return launch_check();
}

int smz_othello_step_ctl(uint64_t *discs_dev, int32_t *mover_dev, const int32_t *action_dev, float *obs_out_dev,
                         float *reward_out_dev, uint8_t *flag_out_dev, const smz_episode_ctl *ctl, double *traj_dev, int T, int t,
                         const double *policy_dev, const double *child_visits_dev, const float *root_value_dev, int B,
                         smz_stream stream) {
    if (!discs_dev || !mover_dev || !action_dev || B < 1) return fail(SMZ_ERR_INVALID, "smz_othello_step_ctl: bad argument%s");
    if (!env_step_args_ok("smz_othello_step_ctl", ctl, traj_dev, policy_dev, child_visits_dev, root_value_dev, T, t))
        return SMZ_ERR_INVALID;
    if (misaligned16(discs_dev)) return fail(SMZ_ERR_INVALID, "smz_othello_step_ctl: discs_dev must be 16-byte aligned%s");
    return launch_board_step(GameOthello{discs_dev, mover_dev}, action_dev, obs_out_dev, reward_out_dev, flag_out_dev, ctl,
                             traj_dev, t, policy_dev, child_visits_dev, root_value_dev, B, stream);
}

int smz_othello_host_step(uint64_t discs[2], int *mover, int action, float *reward_out, int *terminated_out, int *illegal_out) {
    if (!discs || !mover) return fail(SMZ_ERR_INVALID, "smz_othello_host_step: null argument%s");
    uint64_t d0 = discs[0], d1 = discs[1];
    int m = *mover != 0 ? 1 : 0;
    float reward;
    bool over;
    const bool legal = smzoth::play(d0, d1, m, action, reward, over);
    if (legal) {
        discs[0] = d0;
        discs[1] = d1;
        *mover = m;
    }
    if (reward_out) *reward_out = legal ? reward : 0.f;
    if (terminated_out) *terminated_out = over ? 1 : 0;
    if (illegal_out) *illegal_out = legal ? 0 : 1;
    return SMZ_OK;
}

int smz_othello_host_moves(const uint64_t discs[2], int colour, uint64_t *mask_out) {
    if (!discs || !mask_out || (colour != 0 && colour != 1))
        return fail(SMZ_ERR_INVALID, "smz_othello_host_moves: bad argument%s");
    *mask_out = colour ? smzoth::moves(discs[1], discs[0]) : smzoth::moves(discs[0], discs[1]);
    return SMZ_OK;
}

}  // extern "C"
