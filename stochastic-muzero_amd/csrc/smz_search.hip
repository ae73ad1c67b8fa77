// smz_search.hip -- the single-launch mlp_model search for the action buckets 2 and 4 (the headline's unit): the
// instantiations with the trees in global memory, the plain LDS-tree instantiation, KS = 4 and the phase-stamp build, and the
// ABI entry points smz_search_mlp, smz_search_mlp_act and smz_search_mlp_act_cartpole.
#include "smz_search_mlp.hpp"

namespace {
struct NarrowBuckets {
    template <bool INSTR, bool AEX, bool MSK, bool PHX>
    static int launch(const SearchLaunch &s) {
        const int maxa = s.h->maxa;
        if (s.h->K == 2) return maxa == 2 ? s.launch<2, 2, INSTR, AEX, MSK, PHX>() : s.launch<4, 2, INSTR, AEX, MSK, PHX>();
        return maxa == 2 ? s.launch<2, 0, INSTR, AEX, MSK, PHX>() : s.launch<4, 0, INSTR, AEX, MSK, PHX>();
    }
};
}  // namespace

int smz_internal_search_launch_narrow(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev,
                                      int train, SearchActArgs a, const double *pow_table_host, smz_stream stream) {
    if (h && h->maxa > 4) return smz_internal_search_launch_wide(h, desc, weights_dev, obs_dev, train, a, pow_table_host, stream);
    SearchLaunch s = {h, desc, weights_dev, obs_dev, train, a, stream};
    if (const int rc = s.refuse()) return rc;
    DeviceGuard guard(h->cfg.device);
    if (const int rc = s.geometry(pow_table_host)) return rc;
    Params &P = s.P;
    int rc = SMZ_OK;
    {   // LDS-resident trees (k_search_mlp<..., TLDS>): the specialised instantiations -- plain, masked (smz_set_active) and
        // Philox -- when the workgroup's trees fit next to the compact weight image (checkpoint-421 shape, 2 actions: up to
        // ~53 simulations); SMZ_SEARCH_TLDS=0 keeps the trees in global memory (A/B runs)
        const MegaLds mt = mega_lds(*desc, P, s.tpw, true, s.kWaves);
        const size_t lds_t = ((size_t)mt.trees_off + (size_t)s.kWaves * s.tpw * mt.tree_words) * sizeof(float);
        const char *te = getenv("SMZ_SEARCH_TLDS");
        const bool tlds = s.fast && !(P.stats || P.dbg) && h->K == 2 && h->maxa <= 4 && lds_t <= 160 * 1024 && !(te && atoi(te) == 0) &&
                          P.sims <= 126;      // (the block-parallel selection's 7-bit block indices; reachable with 4-wave workgroups only)
#ifdef SMZ_BPS_PROBE
        if (tlds) P.stats = h->d_stats;              // (the production kernel carries no level statistics: only the probe's stamps land there)
#endif
        if (tlds && (P.active || P.philox)) {        // masked / Philox handles: smz_search_lds.hip
            rc = smz_internal_search_launch_tlds(h, desc, weights_dev, obs_dev, train, a, P, s.kWaves, s.blocks, lds_t, stream);
            return rc != SMZ_OK ? rc : search_launched(h);
        }
        if (tlds) {                                  // the plain instantiation (the headline's) stays in this translation unit
#define SMZ_LAUNCH_TLDS(MA)                                                                                            \
            launch_with_lds<k_search_mlp<MA, 2, 1, false, true, false, false, true>>(h, s.blocks, s.threads, lds_t, stream, P, *desc, \
                                                                                     weights_dev, obs_dev, train, s.act(), a.env)
            rc = h->maxa == 2 ? SMZ_LAUNCH_TLDS(2) : SMZ_LAUNCH_TLDS(4);
#undef SMZ_LAUNCH_TLDS
            if (rc != SMZ_OK) return rc;
            name_search_mlp(h, 2, false, true, false, false, true);
            return search_launched(h);
        }
    }
    if ((P.stats || P.dbg) && s.fast && !P.philox && (P.dbg & 32) && h->maxa == 2 && h->K == 2) {
        // phase stamps of the specialised instantiation itself (SMZ_DEBUG_SKIP=48), for the headline geometry only
        hipLaunchKernelGGL((k_search_mlp<2, 2, 1, true, true>), dim3(s.blocks), dim3(s.threads), s.lds, (hipStream_t)stream,
                           P, *desc, weights_dev, obs_dev, train, s.act(), a.env);
        name_search_mlp(h, 2, true, true, true, false, false);
    } else
#if SMZ_KS4
    // Four children per expansion on a four-action tree (SURVEY 8d(3)'s stress shape; round 6): the child count is a compile-time
    // constant (KS = 4: load_kids_static<4>, unrolled scoring, the paired descent on every level) instead of the run-time-K
    // instantiation (KS = 0) -- 347 -> 409 M simulations/s on the K = 4 stress workload, profiles/r06_c_ab_noks4.txt.
    // Plain, masked (smz_set_active) and Philox handles.
    if (s.fast && !(P.stats || P.dbg) && h->maxa == 4 && h->K == 4)
        rc = P.philox ? s.launch<4, 4, false, true, true, true>()
                      : P.active ? s.launch<4, 4, false, true, true, false>() : s.launch<4, 4, false, true, false, false>();
    else
#endif
    rc = s.launch_buckets<NarrowBuckets>();
    return rc != SMZ_OK ? rc : search_launched(h);
}

extern "C" {

int smz_search_mlp(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev, int train,
                   smz_stream stream) {
    if (h && h->large_actions) return refuse_large_actions("smz_search_mlp");
    if (h && h->P.n_cycle > 1) return refuse_multi_player("smz_search_mlp");
    return smz_internal_search_launch_narrow(h, desc, weights_dev, obs_dev, train,
                                             SearchActArgs{0.0, nullptr, nullptr, nullptr, nullptr, EnvStep{}}, nullptr, stream);
}

int smz_search_mlp_act(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev, int train,
                       double temperature, const double *pow_table_host, int32_t *action_dev, double *policy_dev,
                       double *child_visits_dev, float *root_value_dev, smz_stream stream) {
    if (h && h->large_actions) return refuse_large_actions("smz_search_mlp_act");
    if (const int rc = check_act_outputs("smz_search_mlp_act", action_dev, policy_dev, child_visits_dev)) return rc;
    if (h && h->P.n_cycle > 1) return refuse_multi_player("smz_search_mlp_act");
    return smz_internal_search_launch_narrow(h, desc, weights_dev, obs_dev, train,
                                             SearchActArgs{temperature, action_dev, policy_dev, child_visits_dev, root_value_dev,
                                                           EnvStep{}},
                                             pow_table_host, stream);
}

int smz_search_mlp_act_cartpole(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, int train,
                                double temperature, const double *pow_table_host, int32_t *action_dev, double *policy_dev,
                                double *child_visits_dev, float *root_value_dev, const smz_cartpole_env *env,
                                smz_stream stream) {
    if (h && h->large_actions) return refuse_large_actions("smz_search_mlp_act_cartpole");
    if (!action_dev || !policy_dev || !child_visits_dev || !root_value_dev || !env || !env->state_dev || !env->obs_dev)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_act_cartpole: null argument%s");
    if (!h || !desc || h->P.A != 2 || desc->obs != 4)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_act_cartpole: the built-in env has 4 observations and 2 actions%s");
    if (h->P.n_cycle > 1) return refuse_multi_player("smz_search_mlp_act_cartpole");
    const smz_episode_ctl *c = env->ctl;
    if (c && !episode_ctl_ok("smz_search_mlp_act_cartpole", c)) return SMZ_ERR_INVALID;
    if ((c ? c->active_dev : nullptr) != h->P.active)
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_act_cartpole: ctl->active_dev must be the array given to smz_set_active%s");
    if (env->traj_dev && (env->t < 0 || env->t >= env->T))
        return fail(SMZ_ERR_INVALID, "smz_search_mlp_act_cartpole: bad trajectory argument%s");
    if (h->maxa > 4) return fail(SMZ_ERR_INVALID, "smz_search_mlp_act_cartpole: 2 actions%s");
    const EnvStep E = {env->state_dev, env->obs_dev, env->reward_dev, env->flag_dev, c ? c->step_count_dev : nullptr,
                       c ? c->episode_dev : nullptr, c ? c->active_dev : nullptr, c ? c->limit : 0, c ? c->on_end : 0,
                       c ? (uint64_t)c->reset_seed : 0, c ? (long long)c->first_env : 0, env->traj_dev, env->t};
    return smz_internal_search_launch_narrow(h, desc, weights_dev, env->obs_dev, train,
                                             SearchActArgs{temperature, action_dev, policy_dev, child_visits_dev, root_value_dev, E},
                                             pow_table_host, stream);
}

}  // extern "C"
