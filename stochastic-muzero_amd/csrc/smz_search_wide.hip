// smz_search_wide.hip -- the single-launch mlp_model search for the action buckets 8, 16 and 32 (trees in global memory).
#include "smz_search_mlp.hpp"

namespace {
struct WideBuckets {
    template <bool INSTR, bool AEX, bool MSK, bool PHX>
    static int launch(const SearchLaunch &s) {
        const int maxa = s.h->maxa;
        if (s.h->K == 2)
            return maxa == 8 ? s.launch<8, 2, INSTR, AEX, MSK, PHX>()
                             : maxa == 16 ? s.launch<16, 2, INSTR, AEX, MSK, PHX>() : s.launch<32, 2, INSTR, AEX, MSK, PHX>();
        return maxa == 8 ? s.launch<8, 0, INSTR, AEX, MSK, PHX>()
                         : maxa == 16 ? s.launch<16, 0, INSTR, AEX, MSK, PHX>() : s.launch<32, 0, INSTR, AEX, MSK, PHX>();
    }
};
}  // namespace

int smz_internal_search_launch_wide(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev,
                                    int train, SearchActArgs a, const double *pow_table_host, smz_stream stream) {
    SearchLaunch s = {h, desc, weights_dev, obs_dev, train, a, stream};
    if (const int rc = s.refuse()) return rc;
    DeviceGuard guard(h->cfg.device);
    if (const int rc = s.geometry(pow_table_host)) return rc;
    const int rc = s.launch_buckets<WideBuckets>();
    return rc != SMZ_OK ? rc : search_launched(h);
}
