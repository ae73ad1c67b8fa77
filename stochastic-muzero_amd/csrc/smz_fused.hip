// smz_fused.hip -- smz_expand_backup_select: the step-wise expand + backup kernels with the next selection fused in.
#include "smz_common.hpp"
#include "smz_stepwise.hpp"
#include "smz_handle.hpp"

extern "C" {

int smz_expand_backup_select(smz_handle *h, const float *hidden_dev, const float *reward_dev, const float *policy_dev,
                             const float *value_dev, float *parent_hidden_dev, int32_t *last_action_dev,
                             uint8_t *branch_dev, float *mlp_input_dev, smz_stream stream) {
    if (!h || !policy_dev || !value_dev) return fail(SMZ_ERR_INVALID, "smz_expand_backup_select: null argument%s");
    if (!h->selected) return fail(SMZ_ERR_STATE, "smz_expand_backup_select without a preceding smz_select%s");
    DeviceGuard guard(h->cfg.device);
    if (h->large_actions) {      // two launches: the same trees and words as the fused kernel
        const int rc = smz_internal_la_expand_backup(h, hidden_dev, reward_dev, policy_dev, value_dev, stream);
        if (rc != SMZ_OK) return rc;
        return smz_internal_la_select(h, parent_hidden_dev, last_action_dev, branch_dev, mlp_input_dev, stream);
    }
    const bool mp = h->P.n_cycle > 1;      // multi-player handle (smz_set_players)
    if (h->P.philox && h->P.A == h->maxa && h->maxa <= 4) {       // Philox handles, exact action count: the specialised kernel too
#define SMZ_EBS_PHX(KERNEL, MA, KS)                                                                                          \
        hipLaunchKernelGGL((KERNEL<MA, KS, true, true, true>), wave_grid(h->P), dim3(kWave), tree_lds_bytes(h->P),           \
                           (hipStream_t)stream, h->P, hidden_dev, reward_dev, policy_dev, value_dev, parent_hidden_dev,     \
                           last_action_dev, branch_dev, mlp_input_dev)
        if (mp) {
            if (h->maxa == 2) { if (h->K == 2) SMZ_EBS_PHX(k_expand_backup_mp, 2, 2); else SMZ_EBS_PHX(k_expand_backup_mp, 2, 0); }
            else { if (h->K == 2) SMZ_EBS_PHX(k_expand_backup_mp, 4, 2); else SMZ_EBS_PHX(k_expand_backup_mp, 4, 0); }
        } else {
            if (h->maxa == 2) { if (h->K == 2) SMZ_EBS_PHX(k_expand_backup, 2, 2); else SMZ_EBS_PHX(k_expand_backup, 2, 0); }
            else { if (h->K == 2) SMZ_EBS_PHX(k_expand_backup, 4, 2); else SMZ_EBS_PHX(k_expand_backup, 4, 0); }
        }
#undef SMZ_EBS_PHX
        return launch_check();
    }
    if (mp) {
        SMZ_DISPATCH2_AEX(h->maxa, h->K, h->P.A == h->maxa && !h->P.philox, hipLaunchKernelGGL((k_expand_backup_mp<MA, KS, true, AEX>), wave_grid(h->P), dim3(kWave), tree_lds_bytes(h->P),
                                                 (hipStream_t)stream, h->P, hidden_dev, reward_dev, policy_dev, value_dev,
                                                 parent_hidden_dev, last_action_dev, branch_dev, mlp_input_dev));
    } else {
        SMZ_DISPATCH2_AEX(h->maxa, h->K, h->P.A == h->maxa && !h->P.philox, hipLaunchKernelGGL((k_expand_backup<MA, KS, true, AEX>), wave_grid(h->P), dim3(kWave), tree_lds_bytes(h->P),
                                                 (hipStream_t)stream, h->P, hidden_dev, reward_dev, policy_dev, value_dev,
                                                 parent_hidden_dev, last_action_dev, branch_dev, mlp_input_dev));
    }
    return launch_check();
}

}  // extern "C"
