// smz_search_lds.hip -- the masked / Philox instantiations of the single-launch mlp_model search that keep the trees in LDS.
#include "smz_search_mlp.hpp"

// k_search_mlp<MA, 2, 1, false, true, true, PHX, TLDS = true>: masked (smz_set_active) | Philox handles.  The caller
// (smz_internal_search_launch_narrow) has validated everything and computed the geometry.
int smz_internal_search_launch_tlds(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev,
                                    int train, SearchActArgs a, Params P, int kWaves, int blocks, size_t lds_t, smz_stream stream) {
    const ActOut act = {a.temperature, a.action, a.policy, a.child_visits, a.root_value};
#define SMZ_LAUNCH_TLDS(MA, PHX)                                                                                       \
    launch_with_lds<k_search_mlp<MA, 2, 1, false, true, true, PHX, true>>(h, blocks, kWaves * kWave, lds_t, stream, P, *desc, \
                                                                          weights_dev, obs_dev, train, act, a.env)
    const int rc = h->maxa == 2 ? (P.philox ? SMZ_LAUNCH_TLDS(2, true) : SMZ_LAUNCH_TLDS(2, false))
                                : (P.philox ? SMZ_LAUNCH_TLDS(4, true) : SMZ_LAUNCH_TLDS(4, false));
#undef SMZ_LAUNCH_TLDS
    if (rc == SMZ_OK) name_search_mlp(h, 2, false, true, true, P.philox != 0, true);
    return rc;
}
