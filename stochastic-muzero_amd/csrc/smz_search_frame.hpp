// smz_search_frame.hpp -- the device frame the single-launch searches share: what every such kernel does around its own network
// phase and geometry.  Include after smz_common.hpp.
//   * in_vgpr / fresh / unpark: the register-class devices of the kernels that are short of scalar registers
//     (k_search_lstm, k_search_mlp_wide), and pin_search_args, the list of kernel arguments they pin;
//   * stage_pbc: the pb_c table and its reciprocals into LDS (also k_search_mlp_players);
//   * finish_tree: a searched tree's tail -- last expansion + backup, header, (act), stream position (lstm, wide).
// Each kernel keeps its LDS map, its workgroup geometry and barriers, the rounds and the network phase.
#pragma once

namespace {

// A wave-uniform value the per-lane tree code reads, kept in a VECTOR register: a kernel's uniform state (the handle's arrays
// and geometry, the act outputs, the trunk offsets of a network phase) is more than the 100-odd scalar registers of a wave
// hold, and the tree phases use these values in per-lane address arithmetic anyway.  The empty asm only names the register class.
__device__ inline uint32_t in_vgpr(uint32_t v) { asm("" : "+v"(v)); return v; }
__device__ inline int32_t in_vgpr(int32_t v) { return (int32_t)in_vgpr((uint32_t)v); }
__device__ inline float in_vgpr(float v) { return __uint_as_float(in_vgpr(__float_as_uint(v))); }
__device__ inline uint64_t in_vgpr(uint64_t v) { return ((uint64_t)in_vgpr((uint32_t)(v >> 32)) << 32) | in_vgpr((uint32_t)v); }
__device__ inline int64_t in_vgpr(int64_t v) { return (int64_t)in_vgpr((uint64_t)v); }
__device__ inline double in_vgpr(double v) { return __longlong_as_double((long long)in_vgpr((uint64_t)__double_as_longlong(v))); }
template <class T> __device__ inline T *in_vgpr(T *p) { return reinterpret_cast<T *>(in_vgpr((uint64_t)reinterpret_cast<uintptr_t>(p))); }
// ... and a wave-uniform value of a kernel's own loops (trees per wave, the mask of searched tree slots, the round counter) parked
// in a vector register while the per-lane tree code runs -- root_init_tree / expand_backup_tree / select_tree need every scalar
// register a wave has -- and read back where the wave-wide phases start.  (volatile: the read-back is not hoisted out of the
// rounds, which would keep the scalar copy alive across the tree code again.)  fresh: the same for a per-lane value, such as the
// kernels' `valid`: an int compared where it is used; as a bool it would be a lane mask in a scalar register pair for the whole search.
__device__ inline int fresh(int v) { asm volatile("" : "+v"(v)); return v; }
__device__ inline int unpark(int v) { asm volatile("" : "+v"(v)); return __builtin_amdgcn_readfirstlane(v); }

// Every kernel argument the per-lane tree code reads, into vector registers.  static_k: the children per expansion are a
// compile-time constant (KS > 0), so P.K needs no register.  P.S, P.sims, P.B and P.active are pinned by the kernel itself, after
// it has read its scalar copies of them.  A Params field that per-lane code starts to read belongs in this list.
__device__ __forceinline__ void pin_search_args(Params &P, ActOut &act, bool static_k) {
    P.nodes = in_vgpr(P.nodes); P.hdr = in_vgpr(P.hdr); P.path = in_vgpr(P.path); P.mt = in_vgpr(P.mt); P.rng_pos = in_vgpr(P.rng_pos);
    P.pow_table = in_vgpr(P.pow_table); P.rng_block = in_vgpr(P.rng_block); P.rng_key = in_vgpr(P.rng_key);
    P.tree_words = in_vgpr(P.tree_words); P.rb_words = in_vgpr(P.rb_words); P.eb_words = in_vgpr(P.eb_words); P.rp_off = in_vgpr(P.rp_off);
    P.hidden = in_vgpr(P.hidden); P.N = in_vgpr(P.N); P.hs = in_vgpr(P.hs); P.P = in_vgpr(P.P); if (!static_k) P.K = in_vgpr(P.K);
    P.disc32 = in_vgpr(P.disc32); P.keep32 = in_vgpr(P.keep32); P.frac = in_vgpr(P.frac); P.alpha = in_vgpr(P.alpha);
    act.temperature = in_vgpr(act.temperature); act.action = in_vgpr(act.action); act.policy = in_vgpr(act.policy);
    act.child_visits = in_vgpr(act.child_visits); act.root_value = in_vgpr(act.root_value);
}

// The pb_c table of a search of `sims` rounds and, behind it, the reciprocals of the visit counts (select_tree<LUT>), staged by
// the whole workgroup.  The caller's next workgroup barrier publishes them.
__device__ __forceinline__ void stage_pbc(double *pbc_lds, const Params &P, int sims) {
    const int n_pbc = sims + 2;
    for (int i = threadIdx.x; i < n_pbc; i += blockDim.x) {
        pbc_lds[i] = P.pbc_sqrt[i];
        pbc_lds[n_pbc + i] = i > 0 ? 1.0 / (double)i : 0.0;      // IEEE division: correctly rounded reciprocals
    }
}

// The tail of a searched tree, in the tree's lane: the last round's expansion + backup (sims > 0), the header, the post-search
// policy / action when the launch acts, the stream position.  KS: expand_backup_tree's; out: the tree's head outputs (A policy
// values | value | reward); stage: the tree's staged random words; rec: the tree's path records, in their place (path_col).
// (The kernels that keep the path records in LDS and copy the last path back -- k_search_mlp, k_search_vision,
// k_search_mlp_players -- have tails of their own: behind a helper their instruction counts change)
template <int MAXA, int KS, class RNG, class REC>
__device__ __forceinline__ void finish_tree(const Params &P, int tree, RNG &rng, TreeHdr &h, int packed, int sims, const uint32_t *stage,
                                            const float *out, int A, REC rec, const ActOut &act) {
    if (sims > 0) {
        rng.load(P.mt + (size_t)tree * kMtN, packed, stage, kRngStage);
        expand_backup_tree<MAXA, KS>(P, tree, rng, h, out, out[A + 1], out[A], rec);
        packed = rng.pack();
    }
    P.hdr[tree] = h;
    if (act.action) {
        // the post-search policy / action of game.py:179-232 on the finished tree: the same draws from the same stream
        // position as a separate smz_act launch (rng still holds this tree's position)
        act_tree<MAXA>(P, tree, rng, act.temperature, act.action, act.policy, act.child_visits, act.root_value);
        packed = rng.pack();
    }
    P.rng_pos[tree] = packed;
    rng.save(P, tree);
}

}  // namespace
