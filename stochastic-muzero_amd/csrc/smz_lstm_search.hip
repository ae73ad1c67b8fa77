// smz_lstm_search.hip -- the whole Monte_carlo_tree_search.run (mcts:311-349) of every tree in ONE launch for the `lstm_model`
// family: smz_search_lstm / smz_search_lstm_act.
//
// Step-wise, an lstm search is 1 + 2 x simulations launches, and k_lstm_recurrent stages the seven-trunk image (68.5 KB at the
// CartPole shape) into LDS in every workgroup of every launch.  Here a workgroup of four wavefronts stages it ONCE; each
// wavefront then owns `tpw` trees for the whole search:
//   * tree phases (expand + backup of the previous leaf, select) one tree per lane, the per-lane device functions of the
//     step-wise kernels (smz_device.hpp); trees, hidden rows and path records stay in global memory in the handle's layout;
//   * the network phase row by row by the whole wavefront: recurrent_row() of smz_lstm_device.hpp, the row body of
//     k_lstm_recurrent, compiled with the same flags.  The scaled hidden row goes straight into the new node's row of the
//     handle's hidden array; reward, value and policy go to the tree's slot in LDS for the next round's expansion.
// Both paths draw the same random words and round alike: the searches are bit-identical (tests/test_gpu_lstm_search.py).
// The per-lane tree code needs every scalar register a wave has: the kernel's wave-uniform state is pinned or parked in vector
// registers (in_vgpr / unpark / pin_search_args of smz_search_frame.hpp, which also holds the pb_c staging and the tree's tail).
// Limits (anything else runs step-wise): one player, 2 or 4 actions, at most 64 trees per wavefront, LDS map <= 160 KB.
#include "smz_common.hpp"
#include "smz_handle.hpp"
#include "smz_lstm_device.hpp"
#include "smz_search_frame.hpp"

using smz_lstm::kWavesPerWg;
using smz_mlp::lds_sync;
using smz_mlp::up4;

namespace {

constexpr int kWgPerCu = 2;                  // workgroups the geometry puts on a CU before a wave takes a second tree

// LDS map (float offsets from the dynamic LDS base): trunk image | pb_c table + reciprocals (doubles) | the descriptor | per wave: one row's
// scratch | network inputs [tpw][up4(S + A)] | rng tile [tpw][kRngStride] | head outputs [tpw][A + 2] (policy | value | reward)
struct LstmLds {
    int pbc, desc, wave, per_wave, rs, x, rng, outs, total;
};
__host__ __device__ inline LstmLds lstm_lds(const smz_lstm_desc &d, const Params &P, int tpw) {
    LstmLds m;
    m.pbc = r4(d.recurrent_floats);
    m.desc = m.pbc + r4(2 * 2 * (P.sims + 2));
    m.wave = m.desc + r4((int)(sizeof(smz_lstm_desc) / sizeof(float)));
    m.rs = 0;
    m.x = smz_lstm::kRowScratch;
    m.rng = m.x + tpw * up4(d.S + d.A);
    m.outs = m.rng + r4(tpw * kRngStride);
    m.per_wave = m.outs + r4(tpw * (d.A + 2));
    m.total = m.wave + kWavesPerWg * m.per_wave;
    return m;
}

extern __shared__ float4 smz_lsearch_lds4[];

// KS: children per expansion as the step-wise kernels compile it (2: the static two-child block code; 0: run-time K)
template <int MAXA, bool PHX = false, int KS = 0>
__global__ void __launch_bounds__(kWavesPerWg *kWave, kWgPerCu) k_search_lstm(Params Pin, smz_lstm_desc d, const float *__restrict__ weights,
                                                                              const float *__restrict__ hidden0,
                                                                              const float *__restrict__ policy0, int train, ActOut act) {
    Params P = Pin;
    P.tree0 = 0;
    P.philox = PHX ? 1 : 0;                  // (a constant in everything inlined below)
    // the action count equals its bucket (the entry point refuses anything else): the per-action arrays of the tree code stay
    // in registers instead of scratch memory.  (Not d.A: a modified copy of the descriptor, indexed at run time, would live there.)
    P.A = MAXA;
    if (KS > 0) P.K = KS;
    fix_layout(P, true, KS > 0);
    float *lds = reinterpret_cast<float *>(smz_lsearch_lds4);
    pin_search_args(P, act, KS > 0);
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int A = P.A, S = P.S, tpw = P.tpw, sims = P.sims;
    const LstmLds ml = lstm_lds(d, P, tpw);
    P.S = in_vgpr(P.S); P.sims = in_vgpr(P.sims); P.B = in_vgpr(P.B); P.active = in_vgpr(P.active);
    // ---- one-time staging: the seven recurrent trunks, the pb_c table and its reciprocals --------------------------------
    double *pbc_lds = reinterpret_cast<double *>(lds + in_vgpr(ml.pbc));
    stage_pbc(pbc_lds, P, sims);
    // the descriptor too: the network phase reads trunk offsets and layer count from LDS into vector registers (in_vgpr's reason:
    // from the kernel arguments, the fourteen trunk pointers of a round would be hoisted into scalar registers for the whole search)
    static_assert(sizeof(smz_lstm_desc) % sizeof(int32_t) == 0, "descriptor is copied word by word");
    for (int i = threadIdx.x; i < (int)(sizeof(smz_lstm_desc) / sizeof(int32_t)); i += blockDim.x)
        reinterpret_cast<int32_t *>(lds + ml.desc)[i] = reinterpret_cast<const int32_t *>(&d)[i];
    const smz_lstm_desc &dl = *reinterpret_cast<const smz_lstm_desc *>(lds + in_vgpr(ml.desc));
    smz_lstm::stage(lds, weights, d.recurrent_floats);           // (ends with the workgroup barrier; none follows)
    float *wl = lds + in_vgpr(ml.wave + wave * ml.per_wave);
    float *rs = wl + ml.rs, *xall = wl + ml.x, *outs = wl + in_vgpr(ml.outs);
    uint32_t *rng_tile = reinterpret_cast<uint32_t *>(wl + in_vgpr(ml.rng));
    __builtin_assume(rng_tile != nullptr);                       // (the staging helpers test it: as a vector value that test is a lane mask kept for the whole search)
    const int slot = A + 2;

    const int tree0 = in_vgpr((int)(blockIdx.x * kWavesPerWg + wave) * tpw);
    const int tree = tree0 + lane;
    // (an int in a vector register, compared where it is used: as a bool it would be a lane mask in a scalar register pair for the whole search)
    const int valid_v = in_vgpr((lane < tpw && tree < P.B && tree_active(P, tree)) ? 1 : 0);
#define valid (fresh(valid_v) != 0)
    // parked (see unpark): trees per wave | hidden size | rounds | bit t = tree slot t is searched, as two words
    const int tpw_v = in_vgpr(tpw), S_v = in_vgpr(S), sims_v = in_vgpr(sims);
    int vlo_v, vhi_v;
    {
        const unsigned long long vmask = __ballot(valid);
        if (vmask == 0ull) return;                               // beyond B, or every tree switched off (smz_set_active)
        vlo_v = in_vgpr((int)(uint32_t)vmask);
        vhi_v = in_vgpr((int)(uint32_t)(vmask >> 32));
    }
    auto slot_on = [](int lo, int hi, int t) { return (((t < 32 ? lo : hi) >> (t & 31)) & 1) != 0; };

    // ---- root: hidden state and policy come from smz_lstm_initial ---------------------------------------------------------
    {
        const int vlo = unpark(vlo_v), vhi = unpark(vhi_v);
        for (int t = 0; t < tpw; t++) {
            if (!slot_on(vlo, vhi, t)) continue;
            const int row = tree0 + t;
            for (int k = lane; k < S; k += kWave) P.hidden[(size_t)row * P.N * P.hs + k] = hidden0[(size_t)row * S + k];
            if (lane < A) outs[t * slot + lane] = policy0[(size_t)row * A + lane];
        }
    }
    lds_sync();
    int packed = wave_stage_rng<PHX>(P, tree, valid, rng_tile);
    // The root expansion runs in EVERY lane, without a branch on `valid`: a lane that owns no searched tree repeats the work of
    // the wave's first searched slot -- same tree, same staged words, same stream position, in lock step with that lane, so it
    // stores the same values to the same addresses and its own results are never read.  root_init_tree's Dirichlet draws
    // (glibc log / pow) take every scalar register of the wave; the execution mask an `if (valid)` around them would have to
    // keep is the pair that no longer fits.
    RngT<PHX> rng;
    TreeHdr h;
    {
        const int vlo = unpark(vlo_v), vhi = unpark(vhi_v);
        const int first = vlo ? __builtin_ctz((unsigned)vlo) : 32 + __builtin_ctz((unsigned)vhi);    // (one of them is set: see above)
        const int lane_m = valid ? lane : first, tree_m = tree0 + lane_m;
        const int packed_first = __builtin_amdgcn_readlane(packed, first);
        packed = valid ? packed : packed_first;
        rng.bind(P, tree_m, true);
        rng.load(P.mt + (size_t)tree_m * kMtN, packed, rng_tile + lane_m * kRngStride, kRngStage);
        P.sims = unpark(sims_v);            // (root_init_tree branches on it: a uniform branch, no saved execution mask)
        root_init_tree<MAXA>(P, tree_m, rng, outs + lane_m * slot, nullptr, train != 0);
        P.sims = sims_v;
        h = P.hdr[tree_m];
        packed = rng.pack();
    }
    unsigned n_dec = 0, n_chance = 0, n_children = 0;
    // random words are staged once per round, for the NEXT round
    P.tpw = unpark(tpw_v);
    if (unpark(sims_v) > 0) packed = wave_stage_rng_from<4, PHX>(P, tree, valid, rng_tile, packed, rng.block());

    // ---- simulations --------------------------------------------------------------------------------------------------------
    for (int s_v = in_vgpr(0); unpark(s_v) < unpark(sims_v); s_v++) {
        Leaf L = {0, 0, 0, 0};
        if (valid) {
            rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + lane * kRngStride, kRngStage);
            if (s_v > 0) expand_backup_tree<MAXA, KS>(P, tree, rng, h, outs + lane * slot, outs[lane * slot + A + 1], outs[lane * slot + A],
                                                      path_col(P, tree));
            int len = 0;
            L = select_tree<MAXA, KS, false, true>(P, tree, rng, h, pbc_lds, len, n_dec, n_chance, n_children, path_col(P, tree));
            h.path_len = len;
            packed = rng.pack();
        }
        // hidden rows written in earlier rounds (by any lane of this wave) may be this round's parent rows
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        const int ntw = unpark(tpw_v), vlo = unpark(vlo_v), vhi = unpark(vhi_v), Sr = unpark(S_v), K4in = up4(Sr + A);
        // all rows' network inputs first (independent global loads, one latency), then the rows one after another
        for (int t = 0; t < ntw; t++) {
            if (!slot_on(vlo, vhi, t)) continue;
            const int parent = __builtin_amdgcn_readlane(L.parent_id, t), actn = __builtin_amdgcn_readlane(L.action, t);
            const float *src = P.hidden + ((size_t)(tree0 + t) * P.N + parent) * P.hs;
            for (int k = lane; k < K4in; k += kWave)
                xall[t * K4in + k] = (k < Sr) ? src[k] : ((k < Sr + A && (k - Sr) == actn) ? 1.f : 0.f);
        }
        lds_sync();
        for (int t = 0; t < ntw; t++) {
            if (!slot_on(vlo, vhi, t)) continue;                  // a switched-off tree: no network pass
            const int leaf = __builtin_amdgcn_readlane(L.leaf_id, t);
            const bool dyn = __builtin_amdgcn_readlane(L.branch, t) != 0;
            float reward, value;
            smz_lstm::recurrent_row(lds, dl, xall + t * K4in, rs, dyn, lane, P.hidden + ((size_t)(tree0 + t) * P.N + leaf) * P.hs,
                                    outs + t * slot, reward, value);
            if (lane == 0) { outs[t * slot + A] = value; outs[t * slot + A + 1] = reward; }
        }
        lds_sync();
        P.tpw = ntw;
        packed = wave_stage_rng_from<4, PHX>(P, tree, valid, rng_tile, packed, rng.block());
    }
    if (valid)
        finish_tree<MAXA, KS>(P, tree, rng, h, packed, sims_v, rng_tile + lane * kRngStride, outs + lane * slot, A, path_col(P, tree), act);
#undef valid
}

int search_lstm_launch(smz_handle *h, const smz_lstm_desc *desc, const float *weights_dev, const float *hidden0_dev,
                       const float *policy0_dev, int train, ActOut act, const double *pow_table_host, smz_stream stream) {
    if (h && h->large_actions) return refuse_large_actions("smz_search_lstm");
    if (!h || !desc || !weights_dev || !hidden0_dev || !policy0_dev) return fail(SMZ_ERR_INVALID, "smz_search_lstm: null argument%s");
    if (h->P.n_cycle > 1) return refuse_multi_player("smz_search_lstm");
    if (smz_lstm::desc_check(desc, weights_dev) != SMZ_OK)
        return fail(SMZ_ERR_INVALID, "smz_search_lstm: descriptor does not describe an lstm_model weight buffer%s");
    if (desc->A != h->P.A || desc->S != h->P.S)
        return fail(SMZ_ERR_INVALID, "smz_search_lstm: network dimensions differ from the handle's%s");
    if (h->maxa > 4 || h->P.A != h->maxa)
        return fail(SMZ_ERR_TOO_LARGE, "smz_search_lstm: outside the single-launch kernel's limits (2 or 4 actions): use the step-wise entry points%s");
    if (const int rc = check_dirichlet_alpha(h, train)) return rc;
    DeviceGuard guard(h->cfg.device);
    Params P = h->P;
    // two workgroups per CU before a wave takes a second tree
    const int tpw = single_launch_tpw(P.B, kWgPerCu * kCus * kWavesPerWg, nullptr);
    P.tpw = tpw;
    const LstmLds ml = lstm_lds(*desc, P, tpw);
    if (const int rc = check_single_launch_size("smz_search_lstm", tpw, ml.total)) return rc;
    const size_t lds = (size_t)ml.total * sizeof(float);
    if (act.action && use_pow_table(h, P, act.temperature, pow_table_host, stream) != SMZ_OK) return SMZ_ERR_HIP;
    const int blocks = (P.B + kWavesPerWg * tpw - 1) / (kWavesPerWg * tpw), ks = h->K == 2 ? 2 : 0;
#define SMZ_LAUNCH_LS(MA, KK) (P.philox ? SMZ_LAUNCH_LS1(MA, true, KK) : SMZ_LAUNCH_LS1(MA, false, KK))
#define SMZ_LAUNCH_LS1(MA, PX, KK)                                                                                     \
    launch_with_lds<k_search_lstm<MA, PX, KK>>(h, blocks, kWavesPerWg * kWave, lds, stream, P, *desc, weights_dev, hidden0_dev, \
                                               policy0_dev, train, act)
    const int rc = h->maxa == 2 ? (ks ? SMZ_LAUNCH_LS(2, 2) : SMZ_LAUNCH_LS(2, 0)) : (ks ? SMZ_LAUNCH_LS(4, 2) : SMZ_LAUNCH_LS(4, 0));
#undef SMZ_LAUNCH_LS
#undef SMZ_LAUNCH_LS1
    if (rc != SMZ_OK) return rc;
    // (the name as rocprofv3 prints it: without the defaulted arguments)
    if (ks) snprintf(h->last_kernel, sizeof(h->last_kernel), "k_search_lstm<%d, %s, %d>", h->maxa, P.philox ? "true" : "false", ks);
    else snprintf(h->last_kernel, sizeof(h->last_kernel), P.philox ? "k_search_lstm<%d, true>" : "k_search_lstm<%d>", h->maxa);
    return search_launched(h);
}

}  // namespace

extern "C" {

int smz_search_lstm(smz_handle *h, const smz_lstm_desc *desc, const float *weights_dev, const float *hidden0_dev,
                    const float *policy0_dev, int train, smz_stream stream) {
    return search_lstm_launch(h, desc, weights_dev, hidden0_dev, policy0_dev, train, kNoAct, nullptr, stream);
}

int smz_search_lstm_act(smz_handle *h, const smz_lstm_desc *desc, const float *weights_dev, const float *hidden0_dev,
                        const float *policy0_dev, int train, double temperature, const double *pow_table_host,
                        int32_t *action_dev, double *policy_dev, double *child_visits_dev, float *root_value_dev,
                        smz_stream stream) {
    if (const int rc = check_act_outputs("smz_search_lstm_act", action_dev, policy_dev, child_visits_dev)) return rc;
    return search_lstm_launch(h, desc, weights_dev, hidden0_dev, policy0_dev, train,
                              ActOut{temperature, action_dev, policy_dev, child_visits_dev, root_value_dev}, pow_table_host, stream);
}

}  // extern "C"
