// smz_search_mlp.hpp -- the single-launch search of mlp_model trees: its compile-time switches, the kernel k_search_mlp and
// what its launchers share.  The instantiations are split over three translation units (compile time): smz_search.hip holds
// the action buckets 2 and 4 and the ABI entry points, smz_search_wide.hip the buckets 8, 16 and 32, smz_search_lds.hip the
// masked / Philox instantiations with the trees in LDS.
#pragma once
#include "smz_common.hpp"
#include "smz_handle.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Whole search in ONE launch (mlp_model heads): Monte_carlo_tree_search.run (mcts:311-349) for every tree.
// A workgroup = 8 wavefronts sharing one LDS copy of the network weights; a wavefront owns `tpw` trees: the first
// tpw lanes run the per-tree search code (root, select, expand, backup), then all 64 lanes evaluate the networks for
// the wave's leaves one row at a time (smz_mlp_device.hpp).  Leaf/parent hand-off, policies, values and rewards stay
// in LDS; only the child blocks, hidden rows and MT words touch global memory.  No inter-wave communication at all.
// ---------------------------------------------------------------------------------------------------------------
extern __shared__ float4 smz_search_lds4[];

// SMZ_BPS_HBM (round 5): the block-parallel selection also in the specialised kernels whose trees stay in global memory (more
// simulations than LDS holds: BASELINE configs[4]'s per-rank shape) -- every block of a tree is then ONE load from L2 issued by
// its own lane, instead of one dependent L2 round trip per level of the descent
#ifndef SMZ_BPS_HBM
#define SMZ_BPS_HBM 1
#endif
#ifndef SMZ_SELECT_BLOCKS
#define SMZ_SELECT_BLOCKS 1       // block-parallel selection in the kernels that keep their trees in LDS (A/B builds: 0)
#endif
// -DSMZ_BPS_PROBE (variant builds, tools/bps_probe.sh): s_memtime stamps inside the production LDS-resident kernel, summed
// over waves into smz_read_stats' slots 8.. (expand + backup | select: prepare, evaluate, chase, records | networks | staging)
// SMZ_EARLY_ROWS (round 5): in the block-parallel selection the wave's two parent rows are requested from global memory as soon
// as the pointer chase has named them (-DSMZ_EARLY_ROWS=0 builds keep the loads where the network inputs are assembled)
#ifndef SMZ_EARLY_ROWS
#define SMZ_EARLY_ROWS 1
#endif
// SMZ_PAIR_A4 (round 5): the paired descent (two lanes per tree, one child each) for FOUR actions too -- only the root has four
// children, which the two lanes split two and two (pick_decision_pair<Kids<4>>); every level below is the two-action code.
#ifndef SMZ_PAIR_A4
#define SMZ_PAIR_A4 1
#endif
// SMZ_SELECT_TWO_PASSES (round 5): the block-parallel selection on trees in global memory requests the blocks of two passes
// (64 per tree) before it decides the first pass' picks (-DSMZ_SELECT_TWO_PASSES=0: pass by pass; =3: three passes in flight).
#ifndef SMZ_SELECT_TWO_PASSES
#define SMZ_SELECT_TWO_PASSES 1
#endif
#ifndef SMZ_LEAF_FIRST
#define SMZ_LEAF_FIRST 1
#endif
// SMZ_EARLY_STAGE (round 5): the next round's MT19937 source words are requested together with the parent rows -- the stream
// position after the descent follows from the path length alone -- instead of after the selection's last phase.  Before, the
// wait for the (long landed) parent rows at the network inputs was a vmcnt(0) that also waited for the source words requested
// a few instructions earlier: one exposed L2 round trip per round (profiles/r05_s_stage_waits.txt).
#ifndef SMZ_EARLY_STAGE
#define SMZ_EARLY_STAGE 1
#endif
// SMZ_SELECT_MASKS: in the LDS-resident two-action instantiations the path through the evaluated blocks is found without a
// pointer chase -- every block's lane keeps the block's lineage (depth, parent, slot, ancestors as ballot masks) in registers
// and tests it against two ballots (smz_select_masks.hpp); the path records, the leaf and the parent-row requests come from the
// lanes that evaluated the blocks.  Searches of up to 64 simulations (two passes); -DSMZ_SELECT_MASKS=0 builds keep the chase.
#ifndef SMZ_SELECT_MASKS
#define SMZ_SELECT_MASKS 1
#endif
#ifdef SMZ_BPS_PROBE
#define SMZ_PROBE_DECL unsigned long long pb_t0 = 0, pb_acc[7] = {0, 0, 0, 0, 0, 0, 0};
#define SMZ_PROBE_START pb_t0 = __builtin_amdgcn_s_memtime();
#define SMZ_PROBE_AT(i) { const unsigned long long pb_t1 = __builtin_amdgcn_s_memtime(); pb_acc[i] += pb_t1 - pb_t0; pb_t0 = pb_t1; }
// -DSMZ_BPS_PROBE (=1): stamp set A (expand + backup | select: prepare, evaluate, chase, records + leaf | networks | staging);
// -DSMZ_BPS_PROBE=2: set B (expansion | lane-parallel backup | whole select | network inputs (fence, word requests, x rows) |
//                          the two-row pass | head outputs + hand-off | staging) -- same seven slots
#if SMZ_BPS_PROBE + 0 == 2
#define SMZ_PROBE(i)
#define SMZ_PROBE_B(i) SMZ_PROBE_AT(i)
#else
#define SMZ_PROBE(i) SMZ_PROBE_AT(i)
#define SMZ_PROBE_B(i)
#endif
#define SMZ_PROBE_FLUSH(stats) if ((stats) && lane == 0) { for (int pb_i = 0; pb_i < 7; pb_i++) atomicAdd(&(stats)[8 + pb_i], pb_acc[pb_i]); }
#else
#define SMZ_PROBE_DECL
#define SMZ_PROBE_START
#define SMZ_PROBE(i)
#define SMZ_PROBE_B(i)
#define SMZ_PROBE_FLUSH(stats)
#endif

// LDS map of k_search_mlp (floats): weights | pbc table (doubles) | per wave, every part padded to 16 bytes:
//   mlp scratch | network inputs [tpw][K4in] | path records [tpw][P] uint4 | rng tile | head outputs
struct MegaLds {
    int pbc_off, wave_off, per_wave;                       // float offsets from the LDS base
    int x_off, pv_off, rng_off, out_off, sel_off, sel_n;   // float offsets inside a wave's region (sel: block-parallel select)
    int sel_on;                                            // the selection words are there
    int trees_off, tree_words;                             // TLDS: the workgroup's trees (words per tree, blocks packed at 6 K words)
};
// tlds: the instantiation that keeps the workgroup's trees in LDS for the search (and the weights in the compact image)
__host__ __device__ inline MegaLds mega_lds(const smz_mlp_desc &d, const Params &P, int tpw, bool tlds = false, int waves = 8) {
    MegaLds m;
    m.pbc_off = r4(tlds ? smz_mlp::compact_total_floats(d) : d.total_floats - smz_mlp::rep_floats(d));
    m.wave_off = m.pbc_off + r4(2 * 2 * (P.sims + 2));     // pb_c table + reciprocal table (div_by_count)
    m.x_off = r4(2 * smz_mlp::row_scratch_floats(d));     // two rows' scratch: a same-branch pair is evaluated together
    m.pv_off = m.x_off + tpw * smz_mlp::up4(P.S + P.A);
    m.rng_off = m.pv_off + tpw * P.P * 4;
    m.out_off = m.rng_off + r4(tpw * kRngStride);
    m.sel_off = m.out_off + r4(tpw * (P.A + 2));
    m.sel_n = (P.sims + 2 + 1) & ~1;                       // 16-bit words per tree: one per block (select_block / select_chase)
    // (picks per block + the path of the descent: 2 x tpw x sel_n 16-bit words.)  Round 5: the kernels whose trees stay in
    // global memory run the block-parallel selection too (SMZ_BPS_HBM) -- two actions, two children, up to 126 simulations,
    // and only when the words fit beside everything else (host and device evaluate this same function)
    bool sel = tlds;
    if (!tlds && SMZ_BPS_HBM && P.A == 2 && P.K == 2 && tpw == 2 && P.sims <= 126) {
        const int per = m.sel_off + r4(tpw * m.sel_n);
        sel = ((size_t)m.wave_off + (size_t)waves * per) * sizeof(float) <= (size_t)160 * 1024;
    }
    m.sel_on = sel ? 1 : 0;
    m.per_wave = m.sel_off + (sel ? r4(tpw * m.sel_n) : 0);
    m.tree_words = r4(P.rb_words + P.sims * 6 * P.K + (P.K == 2 ? 2 * P.sims : 0));   // (+ the chance thresholds, one double per block;
                                                                                      //  trees stay 16-byte aligned)
    m.trees_off = m.wave_off + waves * m.per_wave;
    return m;
}

// INSTR: instrumented build (level statistics, s_memtime phase stamps, SMZ_DEBUG_SKIP ablations); the production
// instantiation carries none of it -- the accumulators alone cost a dozen scalar registers in a kernel that spills them.
// AEX ("exact"): the specialised instantiation for the common case -- the action count equals the MAXA bucket
// (2, 4, 8, ...), a wavefront owns exactly two trees (the geometry of 4096 trees on 256 CUs) and the networks have the
// shape the reference ships (state_space_dimensions 31, hidden_layer_dimensions 64, number_of_hidden_layer 0: 11 of
// the 16 experiment configs under config/, and checkpoint 421).  A, tpw, K, S, H, L then are compile-time constants for
// everything inlined below: layer loops unroll, and the run-time `j < A` / `t < tpw` / `k < K4` predicates no longer
// live in hoisted 64-bit scalar masks (the generic instantiation spills ~90 SGPRs into VGPR lanes).  Any other
// geometry or shape takes the generic instantiation; both produce identical results (tests/test_gpu_end_to_end.py).
constexpr int kFastTpw = 2, kFastS = 31, kFastH = 64, kFastL = 0;
// MSK: the handle has a per-tree on / off array (smz_set_active).  Without one the validity of a tree slot is a comparison
// that is recomputed where needed; with one it is state that stays live through the search loop -- in the specialised
// instantiation that costs scalar registers it does not have (35 -> 45 spilled, -3 % measured), so it exists both ways.
// PHX: the specialised instantiation for SMZ_RNG_PHILOX handles (counter streams: no state words to load or store).
// TLDS (specialised instantiation, when it fits: ~53 simulations at 2 actions): the workgroup's 16 trees live in LDS for the
// search -- a descent level is an LDS round trip instead of an L2 one, the backup's stores stay on the CU -- and go to their
// place in global memory once, at the end.  LDS room comes from the compact weight image (smz_mlp::mat_op) and from packing
// expansion blocks at 6 K words instead of 64-byte granules.
// (round 6: num_simulations as a ninth, compile-time parameter of the headline instantiation -- LDS map, strides and table offsets
//  as immediates -- measured +0.2 %, inside the spread: profiles/r06_h_sims50_ab.txt; not kept)
template <int MAXA, int KS, int U, bool INSTR, bool AEX, bool MSK = true, bool PHX = false, bool TLDS = false>
__global__ void __launch_bounds__(SMZ_SEARCH_THREADS) k_search_mlp(Params Pin, smz_mlp_desc d, const float *weights, const float *obs,
                                                    int train, ActOut act, EnvStep env) {
    Params P = Pin;
    P.tree0 = 0;
    if (AEX) { P.A = MAXA; P.tpw = kFastTpw; d.A = MAXA; d.S = kFastS; d.H = kFastH; d.L = kFastL; d.OP = smz_mlp::kWave; P.S = kFastS; }
    if (AEX) P.philox = PHX ? 1 : 0;         // (a constant in everything inlined below)
    if (KS > 0) P.K = KS;
    fix_layout(P, AEX, KS > 0);
    if (AEX) P.hs = (kFastS + 15) & ~15;
    float *lds = reinterpret_cast<float *>(smz_search_lds4);
    static_assert(!TLDS || (AEX && KS > 0), "LDS-resident trees: the specialised instantiations only");
    // LDS copy: everything but the representation matrices (TLDS: in the compact image)
    const smz_mlp_desc dl = TLDS ? smz_mlp::lds_desc_compact(d) : smz_mlp::lds_desc_without_rep(d);
    if (TLDS) smz_mlp::stage_weights_compact(lds, weights, d);
    else smz_mlp::stage_weights_without_rep(lds, weights, d);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, waves = blockDim.x / kWave;
    const int A = P.A, S = P.S, tpw = P.tpw;
    const MegaLds ml = mega_lds(d, P, tpw, TLDS, waves);
    uint32_t *const nodes_global = P.nodes;
    const int gl_eb_words = P.eb_words;
    if (TLDS) {       // (compile-time block geometry: every tree access below becomes a ds_* instruction)
        uint32_t *nodes_lds = reinterpret_cast<uint32_t *>(lds + ml.trees_off);
        for (int i = threadIdx.x; i < waves * tpw * ml.tree_words; i += blockDim.x) nodes_lds[i] = 0u;
        P.nodes = nodes_lds;
        P.tree0 = blockIdx.x * waves * tpw;
        P.eb_words = 6 * KS;
        P.tree_words = ml.tree_words;
    }
    // Chance thresholds (select_tree / expand_backup_tree <THR>): in the padding of the 64-byte block when the trees are in
    // global memory, behind the tree's packed blocks when they are in LDS
    // ... and, with the trees in LDS, the children's value terms of the decision-flagged blocks (select_tree<YV>: one division
    // less per decision level; with the trees in global memory the extra store per backup level costs more than it saves:
    // 423 -> 415 M at 4096 x 100)
    constexpr bool THR = AEX && KS == 2, YV = THR && TLDS;
    if (THR) {
        P.thr_off = TLDS ? P.rb_words + P.sims * 6 * KS : P.rb_words + 12;
        P.thr_stride = TLDS ? 2 : P.eb_words;
        P.ry_off = (YV && MAXA <= 8 && P.rp_off + 3 * A <= P.rb_words) ? P.rp_off + 2 * A : -1;      // (select_tree<YV> reads it for MAXA <= 8)
    }
    double *pbc_lds = reinterpret_cast<double *>(lds + ml.pbc_off);
    const int n_pbc = P.sims + 2;
    for (int i = threadIdx.x; i < n_pbc; i += blockDim.x) {
        pbc_lds[i] = P.pbc_sqrt[i];
        pbc_lds[n_pbc + i] = i > 0 ? 1.0 / (double)i : 0.0;      // IEEE division: correctly rounded reciprocals
    }
    const int slot = A + 2;
    const int K4in = smz_mlp::up4(S + A);
    float *scratch = lds + ml.wave_off + wave * ml.per_wave;
    float *xall = scratch + ml.x_off;                                           // [tpw][K4in] network inputs of the round
    uint4 *pvals = reinterpret_cast<uint4 *>(scratch + ml.pv_off);              // [tpw][P] path records
    uint32_t *rng_tile = reinterpret_cast<uint32_t *>(scratch + ml.rng_off);
    float *outs = scratch + ml.out_off;                                         // [tpw][A + 2]: policy | value | reward
    __syncthreads();

    const int tree0 = (blockIdx.x * waves + wave) * tpw;
    const int tree = tree0 + lane;
    const bool valid = lane < tpw && tree < P.B && (!MSK || tree_active(P, tree));
    // a wave none of whose trees is searched (beyond B, or switched off with smz_set_active) is done: there is no
    // workgroup barrier after the weight staging above
    if (MSK && __ballot(valid) == 0ull) {
        // (smz_search_mlp_act_cartpole: the switched-off envs of this wave still get their "no step" record)
        if (env.state && lane < tpw && tree < P.B) cartpole_env_step(env, tree, P.B, act.action, act.policy, act.child_visits, act.root_value);
        return;
    }

    // ---- root: representation + prediction per row, then root expansion per lane ---------------------------------
    for (int t = 0; t < tpw; t++) {
        const int row = tree0 + t;
        if (row >= P.B) break;                                   // wave-uniform
        if (MSK && !__shfl((int)valid, t)) continue;             // wave-uniform: the tree is switched off
        smz_mlp::initial_row<U, TLDS>(lds, dl, weights, d, scratch, obs + (size_t)row * d.obs, P.hidden + (size_t)row * P.N * P.hs,
                                      nullptr, outs + t * slot);
    }
    constexpr bool PHC = !AEX || PHX;   // the specialised instantiations are compiled for one word source each
    int packed = wave_stage_rng<PHC>(P, tree, valid, rng_tile);
    RngT<PHC> rng;
    rng.bind(P, tree, valid);
    TreeHdr h = {0, 0, 0.f, 0.f, 0, 0.f, 0, 0};
    if (valid) {
        rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + lane * kRngStride, kRngStage);
        root_init_tree<MAXA>(P, tree, rng, outs + lane * slot, nullptr, train != 0);
        h = P.hdr[tree];
        packed = rng.pack();
    }
    unsigned n_dec = 0, n_chance = 0, n_children = 0, n_desc = 0;
    // (wave-uniform, read once: inside the rounds a lane picks its tree slot's flag with a select, not a cross-lane read)
    // (one scalar register: the kernel is short of them, and a wave-uniform bool costs a 64-bit lane mask)
    const int vmask = MSK ? __builtin_amdgcn_readlane((int)valid, 0) | (__builtin_amdgcn_readlane((int)valid, 1) << 1) : 3;
#define SMZ_SLOT_VALID(src) (MSK ? ((vmask >> (src)) & 1) != 0 : tree0 + (src) < P.B)
    const bool prof = INSTR && (P.dbg & 16) && P.stats;
    const int dbg = INSTR ? P.dbg : 0;
    unsigned long long t_stage = 0, t_expand = 0, t_select = 0, t_mlp = 0, t0 = 0, t1 = 0;
#define SMZ_STAMP(acc) if (INSTR && prof) { t1 = __builtin_amdgcn_s_memtime(); acc += t1 - t0; t0 = t1; }
    // ---- simulations -------------------------------------------------------------------------------------------------
    // Random words are staged once per round, for the NEXT round: the source words are requested right after the
    // selection (the stream position is final then) and the loads fly during the network evaluation.
    constexpr int SU = 2;
    const bool split = P.tpw <= SU;
    if (P.sims > 0 && !(dbg & 8)) packed = wave_stage_rng_from<4, PHC>(P, tree, valid, rng_tile, packed, rng.block());
    // SMZ_SELECT_MASKS: the lineage of the lane's two blocks (lane >> 1 and 32 + (lane >> 1) of tree slot lane & 1)
    uint32_t lin0 = 0u, lin1 = 0u;                        // smz_masks::lin_pack
    uint64_t anc0 = 0ull, anc1l = 0ull, anc1h = 0ull;   // ancestors: the first block's (pass 0 only), the second's in pass 0 | 1
    SMZ_PROBE_DECL
    for (int s = 0; s < P.sims; s++) {
        if (INSTR && prof) t0 = __builtin_amdgcn_s_memtime();
        SMZ_PROBE_START
        Leaf L = {0, 0, 0, 0};
        __builtin_amdgcn_s_setprio(SMZ_PRIO_TREE);
        // Specialised kernel: the expansion runs in the tree's lane, the backup with one lane per path level
        // (backup_levels_lanes: lanes t, t + 2, ..., t + 14 take eight levels of tree slot t per pass).
        constexpr bool LBKP = AEX && !INSTR;
        float leaf_rw = 0.f;
        if (valid) {
            rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + lane * kRngStride, kRngStage);
            if (s > 0 && !(dbg & 4)) expand_backup_tree<MAXA, KS, LBKP, THR, YV>(P, tree, rng, h, outs + lane * slot, outs[lane * slot + A + 1],
                                                      outs[lane * slot + A], pvals + lane * P.P, &leaf_rw);
        }
        SMZ_PROBE_B(0)
        if constexpr (LBKP) {
            if (s > 0) {
                const int src = lane & (kFastTpw - 1);
                const int len = pick_lane01(h.path_len, src);
                const float lrw = pick_lane01(leaf_rw, src);
                if (lane < 8 * kFastTpw && SMZ_SLOT_VALID(src)) {
                    const bool own = lane < kFastTpw;
                    float mn = own ? h.mn : __builtin_inff(), mx = own ? h.mx : -__builtin_inff(), v_root = 0.f;
                    backup_levels_lanes<kFastTpw, YV>(P, tree0 + src, lane / kFastTpw, len, outs[src * slot + A], lrw,
                                                  pvals + src * P.P, mn, mx, v_root);
                    if (own) {   // the root itself (reward 0)
                        const float nvs = h.root_value_sum + v_root;
                        const int nvc = h.root_visit + 1;
                        h.root_value_sum = nvs;
                        h.root_visit = nvc;
                        const float qv = nvs / (float)nvc;
                        if (qv > mx) mx = qv;
                        if (qv < mn) mn = qv;
                        h.mn = mn;
                        h.mx = mx;
                    }
                }
            }
        }
        SMZ_STAMP(t_expand)
        SMZ_PROBE(0)
        SMZ_PROBE_B(1)
        // Specialised two-action kernel: the descent runs on lanes 0..3 -- lane t and its helper t + 2 score one child
        // each (pick_decision_pair).  The helper works on a copy of the tree lane's stream position and MinMax bounds.
        // (round 6: also four children per block on a four-action tree -- KS = 4: the pair splits EVERY decision level two and
        //  two, pick_decision_pair<Kids<4>>, as it does the root)
        constexpr bool PAIR = AEX && (MAXA == 2 || (SMZ_PAIR_A4 && MAXA == 4)) && (KS == 2 || (SMZ_PAIR_K4 && KS == 4 && MAXA == 4)) && !INSTR;
        // Trees in LDS: block-parallel selection (smz_device.hpp, select_block / select_chase) -- every block of the wave's two
        // trees gets a lane that computes the block's pick from the words its level will read, then the tree's lane follows the
        // picks.  SMZ_SELECT_BLOCKS=0 (-DSMZ_SELECT_BLOCKS=0 builds) keeps the level-by-level descent.
        constexpr bool BPS = SMZ_SELECT_BLOCKS && AEX && KS == 2 && (TLDS || SMZ_BPS_HBM) && !INSTR && MAXA == 2;   // (four actions: the root is a
        // code path of its own beside the blocks' -- measured 409 against 458 M, profiles/r04_bps_ab.txt)
        bool bps_done = false;
        bool bps_all = false;                 // every tree of the wave went through the block-parallel selection this round
        float early_row[kFastTpw] = {0.f, 0.f};
        StagePre<SU> pre;
        bool staged_early = false;            // (wave-uniform) the next round's source words were requested with the parent rows
        // the words the levels of a block-parallel descent of `len` levels drew (all inside the staged window)
        auto descent_words = [&](int len) {
            const int nw = select_words(len, A);
            rng.used += nw; rng.ready -= nw; rng.idx += nw;
            if (rng.idx >= kMtN) { rng.idx -= kMtN; rng.wrapped(); }
            packed = rng.pack();
        };
        // what both block-parallel descents request once the tree's lane knows its path length (0: the tree takes the sequential
        // descent) and can name its leaf's parent node (parent_node(), evaluated by the tree's lane)
        auto early_requests = [&](int len, auto parent_node) {
#if SMZ_EARLY_ROWS
            // Round 5: the leaf's PARENT is known here, before the path records, the leaf's action and the stream position are
            // worked out.  The loads of the wave's two parent rows (global memory: an L2 round trip of ~1.5 k cycles that used
            // to start only after all of that) are issued now and land in registers while the LDS-only rest of the selection
            // runs; the network inputs are written from the registers.  The tree phases of this instantiation touch no global
            // memory, so no later wait of the selection sits behind these loads (gfx950 returns vector-memory loads in order:
            // profiles/r03_ceiling.md 6b).  A tree that falls back to the sequential descent (bps_all false) takes the old path.
            bps_all = __ballot(valid && len == 0) == 0ull && __ballot(valid) != 0ull;
#if SMZ_EARLY_STAGE
            if (valid && len > 0) descent_words(len);
#endif
            if (bps_all) {
                int par = 0;
                if (valid && len > 1) par = parent_node();
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // (rows stored in earlier rounds may be this round's parents)
#pragma unroll
                for (int t = 0; t < kFastTpw; t++) {
                    const int parent = __builtin_amdgcn_readlane(par, t);
                    const float *srow = P.hidden + ((size_t)(tree0 + t) * P.N + parent) * P.hs;
                    early_row[t] = (lane < S && tree0 + t < P.B) ? srow[lane] : 0.f;
                }
#if SMZ_EARLY_STAGE
                if (split && !(dbg & 8)) { stage_issue<SU, PHC>(P, tree, valid, packed, pre); staged_early = true; }
#endif
            }
#endif
        };
        // SMZ_SELECT_MASKS (trees in LDS, at most 64 blocks: two passes): no chase.  Each lane keeps the lineage of its two blocks
        // and finds out from ballots whether they are on this round's path (smz_select_masks.hpp).
        constexpr bool MASKS = SMZ_SELECT_MASKS && BPS && TLDS;
        const bool masks_on = MASKS && P.sims <= smz_masks::kMaxBlocks;      // (wave-uniform; longer searches fit with 4-wave workgroups only)
        if constexpr (MASKS) if (masks_on) {
            namespace mk = smz_masks;
            if (s > 0) {
                // The expansion created block n_exp at depth path_len under the leaf's location (block, slot): the lane that owns
                // the new block takes its lineage -- the parent's ancestors, held by the parent's lane, and the parent itself.
                // All indices are wave-uniform per tree slot.
                int hand = 0;
                if (valid) {
                    const int loc = (int)pvals[lane * P.P + h.path_len - 1].x;
                    hand = h.n_exp | (loc & 0x7f00) | ((loc & 1) << 16) | (h.path_len << 17);
                }
#pragma unroll
                for (int t = 0; t < kFastTpw; t++) {
                    if (!SMZ_SLOT_VALID(t)) continue;
                    const int hw = __builtin_amdgcn_readlane(hand, t);
                    const int e = hw & 255, pb = (hw >> 8) & 255, pl = mk::lane_of(pb, t);
                    const uint64_t q0 = readlane64(anc0, pl), q1l = readlane64(anc1l, pl), q1h = readlane64(anc1h, pl);
                    uint64_t a0, a1;
                    mk::anc_child(pb < 32 ? q0 : q1l, pb < 32 ? 0ull : q1h, pb, t, a0, a1);
                    const uint32_t lin = mk::lin_pack(hw >> 17, pb, (hw >> 16) & 1);
                    if (lane == mk::lane_of(e, t)) {
                        if (e < 32) { lin0 = lin; anc0 = a0; }
                        else { lin1 = lin; anc1l = a0; anc1h = a1; }
                    }
                }
            }
            smz_mlp::lds_sync();
            const int src = lane & 1;
            const int nexp = pick_lane01(valid ? h.n_exp : -1, src), rvis = pick_lane01(h.root_visit, src);
            const float bmn = pick_lane01(h.mn, src), bmx = pick_lane01(h.mx, src);
            const int bused = pick_lane01(valid ? rng.used : 0, src), bstaged = pick_lane01(valid ? rng.staged : 0, src);
            const int bstage = pick_lane01(valid ? (int)(rng.stage - rng_tile) : 0, src);   // the tree's staged words, as its lane reads them
            const int nmax = max(__builtin_amdgcn_readlane(valid ? h.n_exp : -1, 0), __builtin_amdgcn_readlane(valid ? h.n_exp : -1, 1));
            const uint32_t *stb = tree_base(P, tree0 + src);
            SMZ_PROBE(1)
            // per pass: select_block's word (0: the block does not exist or was not evaluated) | the leaf action << 9, and the
            // picked child's (visit, value_sum, reward) -- the words select_record would read back
            uint32_t r0 = 0u, rv0 = 0u, rs0 = 0u, rw0 = 0u, r1 = 0u, rv1 = 0u, rs1 = 0u, rw1 = 0u;
            for (int p = 0; p * (kWave / 2) <= nmax; p++) {
                const int b = p * (kWave / 2) + (lane >> 1);
                uint32_t r = 0u, rv = 0u, rs = 0u, rw = 0u;
                if (b <= nexp) {
                    Kids<2> k;
                    r = select_block_kids<MAXA, YV, RngT<PHC>>(P, stb, b, mk::lin_depth(p ? lin1 : lin0), rvis, bmn, bmx, rng_tile + bstage, bused,
                                                               bstaged, pbc_lds, k);
                    if (r) {
                        const bool pk = (r & 0x80u) != 0u;
                        rv = (uint32_t)(pk ? k.vis[1] : k.vis[0]);
                        rs = __float_as_uint(pk ? k.vsum[1] : k.vsum[0]);
                        rw = __float_as_uint(pk ? k.rew[1] : k.rew[0]);
                        r |= (uint32_t)(b == 0 ? (int)pk : (pk ? k.act[1] : k.act[0])) << 9;       // (the root's child j is action j)
                    }
                }
                if (p == 0) { r0 = r; rv0 = rv; rs0 = rs; rw0 = rw; }
                else { r1 = r; rv1 = rv; rs1 = rs; rw1 = rw; }
            }
            SMZ_PROBE(2)
            const int b0 = lane >> 1, b1 = kWave / 2 + (lane >> 1);
            const uint64_t p0 = __ballot((r0 & 0x80u) != 0u), p1 = __ballot((r1 & 0x80u) != 0u);
            const bool gd0 = b0 <= nexp && mk::good(b0, lin0, src, p0, p1), gd1 = b1 <= nexp && mk::good(b1, lin1, src, p0, p1);
            const uint64_t g0 = __ballot(gd0), g1 = __ballot(gd1);
            const bool on0 = mk::on_path(gd0, anc0, 0ull, g0, g1), on1 = mk::on_path(gd1, anc1l, anc1h, g0, g1);
            const bool ok0 = (r0 & 0x100u) != 0u, ok1 = (r1 & 0x100u) != 0u;
            // a block on the path whose level's words lie beyond the staged window: its tree takes the sequential descent
            const uint64_t fb = __ballot((on0 && !ok0) || (on1 && !ok1));
            // the path's last block: its picked child has no block yet.  Its lane knows the leaf, the path length and the
            // leaf's parent node -- one word, handed to the tree's lane
            const bool lf0 = on0 && ok0 && (r0 & 127u) == 0u, lf1 = on1 && ok1 && (r1 & 127u) == 0u;
            const uint64_t lf = __ballot(lf0 || lf1);
            const uint32_t mine = lf0 ? mk::leaf_pack(b0, lin0, (r0 >> 7) & 1u, (r0 >> 9) & 1u, A) : mk::leaf_pack(b1, lin1, (r1 >> 7) & 1u, (r1 >> 9) & 1u, A);
            uint32_t lw = 0u;
#pragma unroll
            for (int t = 0; t < kFastTpw; t++) {
                const int ll = mk::leaf_lane(lf, t);
                if ((fb & mk::tree_lanes(t)) == 0ull && ll >= 0) {
                    const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)mine, ll);
                    if (lane == t) lw = w;
                }
            }
            const int len = valid ? mk::leaf_len(lw) : 0;
            SMZ_PROBE(3)
            early_requests(len, [&] { return mk::leaf_parent(lw); });
            // the path records, from the registers of the lanes on the path (record d: the block at depth d)
            if ((fb & mk::tree_lanes(src)) == 0ull) {
                if (on0) pvals[src * P.P + mk::lin_depth(lin0)] = make_uint4((uint32_t)(b0 << 8) | ((r0 >> 7) & 1u), rv0, rs0, rw0);
                if (on1) pvals[src * P.P + mk::lin_depth(lin1)] = make_uint4((uint32_t)(b1 << 8) | ((r1 >> 7) & 1u), rv1, rs1, rw1);
            }
            if (valid && len > 0) {
                const int loc = mk::leaf_loc(lw);
                L.leaf_id = mk::child_node(loc >> 8, loc & 1, A);
                L.parent_id = len > 1 ? mk::leaf_parent(lw) : 0;
                L.action = mk::leaf_action(lw);
                L.branch = depth_flag(len - 1);
#if !(SMZ_EARLY_ROWS && SMZ_EARLY_STAGE)
                descent_words(len);
#endif
                h.path_len = len;
                bps_done = true;
            }
        }
        if constexpr (BPS) if (!masks_on && (TLDS || ml.sel_on)) {
            uint16_t *selw = reinterpret_cast<uint16_t *>(scratch + ml.sel_off);          // [tpw][sel_n]
            const int SELN = ml.sel_n;
            if (valid && s > 0) selw[lane * SELN + h.n_exp] = (uint16_t)(h.path_len << 9);   // depth of the node the expansion created
            smz_mlp::lds_sync();
            const int src = lane & 1;
            const int nexp = pick_lane01(valid ? h.n_exp : -1, src), rvis = pick_lane01(h.root_visit, src);
            const float bmn = pick_lane01(h.mn, src), bmx = pick_lane01(h.mx, src);
            const int bused = pick_lane01(valid ? rng.used : 0, src), bstaged = pick_lane01(valid ? rng.staged : 0, src);
            const int bstage = pick_lane01(valid ? (int)(rng.stage - rng_tile) : 0, src);   // the tree's staged words, as its lane reads them
            const int nmax = max(__builtin_amdgcn_readlane(valid ? h.n_exp : -1, 0), __builtin_amdgcn_readlane(valid ? h.n_exp : -1, 1));
            const uint32_t *stb = tree_base(P, tree0 + src);
            SMZ_PROBE(1)
            if constexpr (!TLDS && SMZ_SELECT_LOADS_FIRST && SMZ_SELECT_TWO_PASSES) {
                // Trees in global memory: a pass of 32 blocks per tree is one L2 round trip, and a search of 100 simulations takes
                // up to four of them one after the other.  The blocks of TWO passes are requested before the first is decided.
                constexpr int NP = SMZ_SELECT_TWO_PASSES > 1 ? SMZ_SELECT_TWO_PASSES : 2;          // passes in flight
                for (int base = 0; base <= nmax; base += NP * (kWave / 2)) {
                    BlockRaw raw[NP];
#pragma unroll
                    for (int p = 0; p < NP; p++) {
                        const int b = base + p * (kWave / 2) + (lane >> 1);
                        if (b <= nexp) select_block_request<MAXA, YV>(P, stb, b, raw[p]);
                    }
#pragma unroll
                    for (int p = 0; p < NP; p++) {
                        const int b = base + p * (kWave / 2) + (lane >> 1);
                        if (b <= nexp) {
                            const int depth = b == 0 ? 0 : (int)(selw[src * SELN + b] >> 9);
                            const uint32_t r = select_block_decide<MAXA, YV, RngT<PHC>>(P, b, depth, rvis, bmn, bmx, rng_tile + bstage, bused, bstaged,
                                                                                         pbc_lds, raw[p]);
                            selw[src * SELN + b] = (uint16_t)((depth << 9) | r);
                        }
                    }
                }
            } else
            for (int base = 0; base <= nmax; base += kWave / 2) {
                const int b = base + (lane >> 1);
                if (b <= nexp) {
                    const int depth = b == 0 ? 0 : (int)(selw[src * SELN + b] >> 9);
                    const uint32_t r = select_block<MAXA, YV, RngT<PHC>, !TLDS>(P, stb, b, depth, rvis, bmn, bmx, rng_tile + bstage, bused, bstaged,
                                                                        pbc_lds);
                    selw[src * SELN + b] = (uint16_t)((depth << 9) | r);
                }
            }
            smz_mlp::lds_sync();
            SMZ_PROBE(2)
            // the descent: the tree's lane follows the picks (one dependent LDS read per level) and leaves the path in the upper half
            // of the tree's sel words (sel_n covers both); then one lane per level writes that level's path record.
            // (The same chase on the scalar unit -- picks kept in the lanes that computed them, a v_readlane per level, path entries
            // dropped into lanes by compare + select, no LDS traffic -- was built twice: round 4 at the 256-register limit (-8 %,
            // scratch) and round 5 with 58 registers to spare (-4 %: 106 scalar registers are the limit too, and a taken scalar
            // branch per level costs what the LDS round trip does); profiles/r05_f_pair_chase_ab.txt, commit "experiment: scalar
            // chase".)
            uint16_t *pathw = selw + tpw * SELN;                                        // [tpw][sel_n]
            int len = 0;
            if (valid) len = select_chase(selw + lane * SELN, pathw + lane * SELN);
            smz_mlp::lds_sync();
            SMZ_PROBE(3)
            const int blen = pick_lane01(len, src);
            early_requests(len, [&] { const int loc = pathw[lane * SELN + len - 2], pb = loc >> 8; return pb == 0 ? 1 + (loc & 3) : 1 + A + (pb - 1) * 2 + (loc & 3); });
            // (trees in global memory: the leaf's action word is requested BEFORE the path records' words, so the two L2 round trips
            //  overlap -- the records' loop waits for its own loads, and the leaf's used to start only behind that wait)
            if constexpr (!TLDS && SMZ_LEAF_FIRST) { if (valid && len > 0) L = select_leaf(P, stb, pathw + lane * SELN, len); }
            for (int d = lane >> 1; d < blen; d += kWave / 2) select_record(P, stb, pathw + src * SELN, d, pvals + src * P.P);
            if (valid && len > 0) {
                if constexpr (TLDS || !SMZ_LEAF_FIRST) L = select_leaf(P, stb, pathw + lane * SELN, len);
#if !(SMZ_EARLY_ROWS && SMZ_EARLY_STAGE)
                descent_words(len);
#endif
                h.path_len = len;
                bps_done = true;
            }
        }
        if constexpr (BPS) {
            // (a level's words beyond the staged window -- a very deep path, or a window nearly used up: the sequential descent)
            if (valid && !bps_done) {
                int len = 0;
                L = select_tree<MAXA, KS, false, true, false, THR, YV>(P, tree, rng, h, pbc_lds, len, n_dec, n_chance, n_children, pvals + lane * P.P);
                h.path_len = len;
                packed = rng.pack();
            }
        } else if constexpr (PAIR) {
            const int src = lane & 1;
            const int pk = pick_lane01(valid ? rng.pack() : 0, src), us = pick_lane01(valid ? rng.used : 0, src);

            const float hmn = pick_lane01(h.mn, src), hmx = pick_lane01(h.mx, src);
            const int hrv = pick_lane01(h.root_visit, src);
            const uint32_t pb = (uint32_t)pick_lane01((int)rng.block(), src), pk0 = (uint32_t)pick_lane01((int)rng.key0(), src),
                           pk1 = (uint32_t)pick_lane01((int)rng.key1(), src);
            if (lane < 4 && SMZ_SLOT_VALID(src)) {
                TreeHdr hs = h;
                if (lane >= 2) {
                    rng.load(P.mt + (size_t)(tree0 + src) * kMtN, pk, rng_tile + src * kRngStride, kRngStage);
                    rng.used = us;
                    rng.follow(pb, pk0, pk1);      // (Philox: the helper draws beyond the staged window from the TREE's stream)
                    hs.mn = hmn; hs.mx = hmx; hs.root_visit = hrv;
                }
                int len = 0;
                const Leaf Lp = select_tree<MAXA, KS, false, true, true, THR, YV>(P, tree0 + src, rng, hs, pbc_lds, len, n_dec, n_chance,
                                                                             n_children, pvals + src * P.P, lane >> 1);
                if (lane < 2) {
                    L = Lp;
                    h.path_len = len;
                    packed = rng.pack();
                }
            }
        } else if (valid) {
            int len = 0;
            if (dbg & 2) { L.leaf_id = 1; L.parent_id = 0; L.action = 0; L.branch = 0; len = 1; }
            else L = select_tree<MAXA, KS, INSTR, true, false, THR, YV>(P, tree, rng, h, pbc_lds, len, n_dec, n_chance, n_children, pvals + lane * P.P);
            h.path_len = len;
            if (INSTR) n_desc++;
            packed = rng.pack();
        }
        SMZ_STAMP(t_select)
        SMZ_PROBE(4)
        SMZ_PROBE_B(2)
        __builtin_amdgcn_s_setprio(SMZ_PRIO_HEADS);
        // hidden rows written in earlier rounds (by any lane of this wave) may be this round's parent rows
        if (!(BPS && SMZ_EARLY_ROWS && bps_all)) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        // (after the fence: it drains the vector-memory counter)
        if (split && !(dbg & 8) && !staged_early) stage_issue<SU, PHC>(P, tree, valid, packed, pre);
        // all rows' network inputs first (independent global loads, one latency), then the rows one after another
        if (BPS && SMZ_EARLY_ROWS && bps_all) {                 // (the parent rows are in registers already: see the selection)
#pragma unroll
            for (int t = 0; t < kFastTpw; t++) {
                if (tree0 + t >= P.B) break;
                const int act = __builtin_amdgcn_readlane(L.action, t);
                if (lane < K4in) xall[t * K4in + lane] = (lane < S) ? early_row[t] : ((lane < S + A && (lane - S) == act) ? 1.f : 0.f);
            }
        } else
        for (int t = 0; t < tpw; t++) {
            const int row = tree0 + t;
            if (row >= P.B) break;                               // wave-uniform
            const int parent = __builtin_amdgcn_readlane(L.parent_id, t), act = __builtin_amdgcn_readlane(L.action, t);
            const float *src = P.hidden + ((size_t)row * P.N + parent) * P.hs;
            for (int k = lane; k < K4in; k += kWave)
                xall[t * K4in + k] = (k < S) ? src[k] : ((k < S + A && (k - S) == act) ? 1.f : 0.f);
        }
        smz_mlp::lds_sync();
        SMZ_PROBE_B(3)
        bool paired = false;
        if (tpw == 2 && !(dbg & 1)) {
            // the wave's two leaves need the same pair of networks: one pass, weights read from LDS once for both rows
            const int b0 = __builtin_amdgcn_readlane(L.branch, 0), b1 = __builtin_amdgcn_readlane(L.branch, 1);
            if (tree0 + 1 < P.B) {
                const float *xin[2] = {xall, xall + K4in};
                const bool dyn[2] = {b0 != 0, b1 != 0};
                float *dh[2], *dp[2] = {outs, outs + slot};
                float reward[2], value[2];
#pragma unroll
                for (int r = 0; r < 2; r++)
                    dh[r] = P.hidden + ((size_t)(tree0 + r) * P.N + __builtin_amdgcn_readlane(L.leaf_id, r)) * P.hs;
                const bool live[2] = {MSK ? (vmask & 1) != 0 : true, MSK ? (vmask & 2) != 0 : true};
                if (b0 == b1) smz_mlp::recurrent_rows<U, 2, true, TLDS>(lds, dl, scratch, xin, dyn, live, dh, dp, reward, value);
                else smz_mlp::recurrent_rows<U, 2, false, TLDS>(lds, dl, scratch, xin, dyn, live, dh, dp, reward, value);
                SMZ_PROBE_B(4)
                if (lane == 0) {
                    outs[A] = value[0]; outs[A + 1] = reward[0];
                    outs[slot + A] = value[1]; outs[slot + A + 1] = reward[1];
                }
                paired = true;
            }
        }
        for (int t = 0; t < tpw && !paired; t += smz_mlp::kRows) {
            if (tree0 + t >= P.B) break;                         // wave-uniform
            constexpr int R = smz_mlp::kRows;
            const float *xin[R];
            bool dyn[R], live[R];
            float *dh[R], *dp[R];
            float reward[R], value[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                live[r] = (t + r < tpw) && (tree0 + t + r < P.B);
                const int tt = live[r] ? t + r : t;
                live[r] = live[r] && (!MSK || __shfl((int)valid, tt) != 0);
                const int row = tree0 + tt;
                const int leaf = __builtin_amdgcn_readlane(L.leaf_id, tt);
                dyn[r] = __builtin_amdgcn_readlane(L.branch, tt) != 0;
                xin[r] = xall + tt * K4in;
                dh[r] = P.hidden + ((size_t)row * P.N + leaf) * P.hs;
                dp[r] = outs + tt * slot;
            }
            if (!(dbg & 1)) smz_mlp::recurrent_rows<U, R, false, TLDS>(lds, dl, scratch, xin, dyn, live, dh, dp, reward, value);
#pragma unroll
            for (int r = 0; r < R; r++)
                if (live[r] && lane == 0) { outs[(t + r) * slot + A] = value[r]; outs[(t + r) * slot + A + 1] = reward[r]; }
        }
        smz_mlp::lds_sync();
        SMZ_STAMP(t_mlp)
        SMZ_PROBE(5)
        SMZ_PROBE_B(5)
        if (!(dbg & 8)) packed = split ? stage_finish<SU, PHC>(P, tree, valid, rng_tile, packed, pre, rng.block())
                                       : wave_stage_rng_from<4, PHC>(P, tree, valid, rng_tile, packed, rng.block());
        SMZ_STAMP(t_stage)
        SMZ_PROBE(6)
        SMZ_PROBE_B(6)
    }
    SMZ_PROBE_FLUSH(Pin.stats)
#undef SMZ_STAMP
#undef SMZ_SLOT_VALID
    if (INSTR && prof && lane == 0) {
        atomicAdd(&P.stats[4], t_stage); atomicAdd(&P.stats[5], t_expand);
        atomicAdd(&P.stats[6], t_select); atomicAdd(&P.stats[7], t_mlp);
    }
    if (valid) {
        if (P.sims > 0) {
            rng.load(P.mt + (size_t)tree * kMtN, packed, rng_tile + lane * kRngStride, kRngStage);
            expand_backup_tree<MAXA, KS, false, THR, YV>(P, tree, rng, h, outs + lane * slot, outs[lane * slot + A + 1], outs[lane * slot + A],
                                                     pvals + lane * P.P);
            // leave the last path where the step-wise entry points and the debug dump expect it
            for (int i = 0; i < h.path_len; i++) P.path[(size_t)i * P.B + tree] = pvals[lane * P.P + i];
            packed = rng.pack();
        }
        P.hdr[tree] = h;
        if (act.action) {
            // the post-search policy / action of game.py:179-232 on the finished tree: the same draws from the same
            // stream position as a separate smz_act launch (rng still holds this tree's position)
            act_tree<MAXA>(P, tree, rng, act.temperature, act.action, act.policy, act.child_visits, act.root_value);
            packed = rng.pack();
        }
        P.rng_pos[tree] = packed;
        rng.save(P, tree);
    }
    if constexpr (TLDS) {
        // the wave's finished trees back to their place in global memory (64-byte granules there: words 12..15 of a block are
        // padding).  Each wave moves its own trees: no other wave has touched them.
        smz_mlp::lds_sync();
        const int n_blk = 1 + P.sims;                                    // root block + one expansion block per simulation
        for (int t = 0; t < tpw; t++) {
            if (tree0 + t >= P.B) break;
            if (MSK && !__shfl((int)valid, t)) continue;             // a switched-off tree keeps what its last search left in HBM
            const uint32_t *src = P.nodes + (size_t)(wave * tpw + t) * P.tree_words;
            uint32_t *dst = nodes_global + (size_t)(tree0 + t) * (P.rb_words + (size_t)P.sims * gl_eb_words);
            for (int i = lane; i < P.rb_words; i += kWave) dst[i] = src[i];
            for (int i = lane; i < (n_blk - 1) * gl_eb_words; i += kWave) {
                const int b = i / gl_eb_words, w = i - b * gl_eb_words;
                dst[P.rb_words + i] = w < P.eb_words ? src[P.rb_words + b * P.eb_words + w] : 0u;
            }
        }
    }
    // smz_search_mlp_act_cartpole: the env step + trajectory record of this tree's env in the same lane (it reads back
    // the action / policy / child_visits / root value it has just written); a switched-off tree of a live wave gets its
    // "no step" record.  The next observation goes where this launch read the current one: only this wave reads that row.
    if (env.state && lane < tpw && tree < P.B)
        cartpole_env_step(env, tree, P.B, act.action, act.policy, act.child_visits, act.root_value);
    if (INSTR) wave_add_stats(P.stats, n_dec, n_chance, n_desc, n_children);
}

}  // namespace

struct SearchActArgs {       // ActOut (+ the fused env step) across the translation-unit boundary (plain data)
    double temperature;
    int32_t *action;
    double *policy, *child_visits;
    float *root_value;
    EnvStep env;             // env.state == nullptr: no env step in the launch
};

// smz_last_kernel's text for an instantiation of the handle's action bucket, as rocprofv3 prints it (U = 1 everywhere)
static void name_search_mlp(smz_handle *h, int ks, bool instr, bool aex, bool msk, bool phx, bool tlds) {
    const auto b = [](bool v) { return v ? "true" : "false"; };
    snprintf(h->last_kernel, sizeof(h->last_kernel), "k_search_mlp<%d, %d, 1, %s, %s, %s, %s, %s>", h->maxa, ks, b(instr), b(aex),
             b(msk), b(phx), b(tlds));
}
int smz_internal_search_launch_narrow(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev,
                                      int train, SearchActArgs a, const double *pow_table_host, smz_stream stream);
int smz_internal_search_launch_wide(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev,
                                    int train, SearchActArgs a, const double *pow_table_host, smz_stream stream);
// smz_search_lds.hip: the masked / Philox instantiations that keep the workgroup's trees in LDS (P, geometry and LDS size come
// from the caller)
int smz_internal_search_launch_tlds(smz_handle *h, const smz_mlp_desc *desc, const float *weights_dev, const float *obs_dev,
                                    int train, SearchActArgs a, Params P, int kWaves, int blocks, size_t lds_t, smz_stream stream);

// ---- what the narrow and the wide launcher share ----
namespace {

struct SearchLaunch {
    // the launcher's arguments
    smz_handle *h;
    const smz_mlp_desc *desc;
    const float *weights_dev, *obs_dev;
    int train;
    SearchActArgs a;
    smz_stream stream;
    // the geometry of the launch (geometry())
    Params P;                 // the handle's, with this launch's trees per wave and power table
    int kWaves, tpw, blocks, threads;
    size_t lds;
    bool fast;                // the specialised (AEX) instantiations apply

    // The refusals that come before the device guard.
    int refuse() const {
        if (!h || !desc || !weights_dev || !obs_dev) return fail(SMZ_ERR_INVALID, "smz_search_mlp: null argument%s");
        smz_mlp_desc t = *desc;
        if (smz_mlp_layout(&t) != SMZ_OK || t.total_floats != desc->total_floats)
            return fail(SMZ_ERR_INVALID, "smz_search_mlp: descriptor does not describe an LDS-resident network%s");
        if (desc->A != h->P.A || desc->S != h->P.S)
            return fail(SMZ_ERR_INVALID, "smz_search_mlp: network dimensions differ from the handle's%s");
        return check_dirichlet_alpha(h, train);
    }

    // Under the caller's device guard: the geometry, the last refusal (the LDS size), then the power table of a launch that acts.
    int geometry(const double *pow_table_host) {
        kWaves = 8;
        if (const char *e = getenv("SMZ_SEARCH_WAVES")) { const int v = atoi(e); if ((v == 1 || v == 2 || v == 4 || v == 8 || v == 12 || v == 16) && v * kWave <= SMZ_SEARCH_THREADS) kWaves = v; }
        P = h->P;
        // trees per wave: the smallest power of two that covers B with 256 workgroups of 8 waves, capped at 2 -- beyond
        // 4096 trees the grid simply has more workgroups than CUs and they run one after another (each re-stages the
        // weights, ~1 % of its run time): per-wave LDS buffers stay small and the specialised instantiation applies.
        tpw = 1;
        while (tpw < kFastTpw && (size_t)256 * kWaves * tpw < (size_t)P.B) tpw <<= 1;
        if (const char *e = getenv("SMZ_SEARCH_TPW")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) tpw = v; }
        P.tpw = tpw;
        const MegaLds ml = mega_lds(*desc, P, tpw, false, kWaves);
        const long long lds_floats = (long long)ml.wave_off + (long long)kWaves * ml.per_wave;
        if (const int rc = check_single_launch_size("smz_search_mlp", tpw, lds_floats)) return rc;
        lds = (size_t)lds_floats * sizeof(float);
        if (a.action && use_pow_table(h, P, a.temperature, pow_table_host, stream) != SMZ_OK) return SMZ_ERR_HIP;
        blocks = (P.B + kWaves * tpw - 1) / (kWaves * tpw);
        threads = kWaves * kWave;
        // (the specialised instantiation is the parity-mode path: a Philox handle runs the generic one)
        fast = P.A == h->maxa && tpw == kFastTpw && desc->S == kFastS && desc->H == kFastH && desc->L == kFastL;
        return SMZ_OK;
    }

    ActOut act() const { return ActOut{a.temperature, a.action, a.policy, a.child_visits, a.root_value}; }

    // One instantiation with the trees in global memory, and its name for smz_last_kernel.
    template <int MA, int KS, bool INSTR, bool AEX, bool MSK, bool PHX>
    int launch() const {
        const int rc = launch_with_lds<k_search_mlp<MA, KS, 1, INSTR, AEX, MSK, PHX>>(h, blocks, threads, lds, stream, P, *desc, weights_dev,
                                                                                     obs_dev, train, act(), a.env);
        if (rc == SMZ_OK) name_search_mlp(h, KS, INSTR, AEX, MSK, PHX, false);
        return rc;
    }

    // The five instantiations of every action bucket.  smz_mlp_layout only accepts OP == 64 (one output neuron per lane): U = 1.
    // The instrumented instantiation runs when level statistics are enabled (smz_enable_stats) or a SMZ_DEBUG_SKIP switch is set.
    // Buckets::launch<INSTR, AEX, MSK, PHX>(s) picks the handle's (MA, KS) among the unit's buckets and calls s.launch<MA, KS, ...>.
    // (The choice among the five is the outer one on purpose: the kernels are instantiated, and so laid out in the unit, in
    // this order, and the wide buckets' kernels call out-of-line functions whose inlining follows that order.)
    template <class Buckets>
    int launch_buckets() const {
        if (P.stats || P.dbg) return Buckets::template launch<true, false, true, false>(*this);
        if (fast && P.philox) return Buckets::template launch<false, true, true, true>(*this);
        if (fast && !P.active) return Buckets::template launch<false, true, false, false>(*this);
        if (fast) return Buckets::template launch<false, true, true, false>(*this);
        return Buckets::template launch<false, false, true, false>(*this);
    }
};

}  // namespace
