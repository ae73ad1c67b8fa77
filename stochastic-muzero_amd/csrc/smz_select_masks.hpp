// smz_select_masks.hpp -- the bit logic of the mask-based path membership of the block-parallel selection (SMZ_SELECT_MASKS).
//
// The block-parallel selection gives every block of a wavefront's two trees a lane: lane l owns blocks l >> 1 and 32 + (l >> 1)
// of tree slot l & 1, one per pass.  A ballot over a pass therefore carries block b of tree slot t at bit 2 (b & 31) + t of the
// pass-(b >> 5) ballot -- "lane space".  A block's parent, the slot it hangs from and its ancestors never change after the
// expansion that created it, so its lane can keep them in registers, the ancestors as masks in lane space.  Then
//     good(b)    = the parent's pick equals b's slot                    (one bit test against the ballot of the picks)
//     on path(b) = good(b) and every ancestor of b is good              (two mask tests against the ballots of good)
// and the descent needs no dependent chain over the picks.  Plain integers only: the kernel (smz_search_mlp.hpp) and a host test
// (tests/test_select_masks.py) compile this same file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMZ_MASKS_HD __host__ __device__
#else
#define SMZ_MASKS_HD
#endif

namespace smz_masks {

constexpr int kMaxBlocks = 64;                           // two passes of 32 blocks per tree slot

SMZ_MASKS_HD inline int lane_of(int b, int tslot) { return 2 * (b & 31) + tslot; }        // the lane that owns block b = its ballot bit
SMZ_MASKS_HD inline int pass_of(int b) { return b >> 5; }
SMZ_MASKS_HD inline uint64_t bit_of(int b, int tslot) { return (uint64_t)1 << lane_of(b, tslot); }
SMZ_MASKS_HD inline uint64_t tree_lanes(int tslot) { return (uint64_t)0x5555555555555555ull << tslot; }   // every lane of one tree slot

// lineage word of a block: depth of its node | parent block << 8 | slot in the parent << 16 (the root: 0)
SMZ_MASKS_HD inline uint32_t lin_pack(int depth, int parent, int slot) { return (uint32_t)depth | ((uint32_t)parent << 8) | ((uint32_t)slot << 16); }
SMZ_MASKS_HD inline int lin_depth(uint32_t lin) { return (int)(lin & 0xffu); }
SMZ_MASKS_HD inline int lin_parent(uint32_t lin) { return (int)((lin >> 8) & 0xffu); }
SMZ_MASKS_HD inline int lin_slot(uint32_t lin) { return (int)((lin >> 16) & 1u); }

// ancestors of a block created under block pb: the parent's ancestors and the parent itself (a0: pass-0 ballot, a1: pass 1)
SMZ_MASKS_HD inline void anc_child(uint64_t pa0, uint64_t pa1, int pb, int tslot, uint64_t &a0, uint64_t &a1) {
    a0 = pa0; a1 = pa1;
    if (pass_of(pb) == 0) a0 |= bit_of(pb, tslot);
    else a1 |= bit_of(pb, tslot);
}

// p0, p1: the ballots of the picks of pass 0 / 1.  The root is always good.
SMZ_MASKS_HD inline bool good(int b, uint32_t lin, int tslot, uint64_t p0, uint64_t p1) {
    if (b == 0) return true;
    const int pb = lin_parent(lin);
    const uint64_t pp = pass_of(pb) == 0 ? p0 : p1;
    return (int)((pp >> lane_of(pb, tslot)) & 1u) == lin_slot(lin);
}
// g0, g1: the ballots of good (blocks that do not exist contribute nothing)
SMZ_MASKS_HD inline bool on_path(bool is_good, uint64_t a0, uint64_t a1, uint64_t g0, uint64_t g1) {
    return is_good && ((a0 & ~g0) | (a1 & ~g1)) == 0;
}

// node id of the node that owns block b (the reference's creation-order ids: root 0, root children 1 .. A, children of block
// pb >= 1 at 1 + A + (pb - 1) 2 + slot), and of the child in slot `pick` of block b
SMZ_MASKS_HD inline int child_node(int b, int pick, int A) { return b == 0 ? 1 + pick : 1 + A + (b - 1) * 2 + pick; }
SMZ_MASKS_HD inline int owner_node(int b, uint32_t lin, int A) { return b == 0 ? 0 : child_node(lin_parent(lin), lin_slot(lin), A); }

// What the lane of the path's last block hands to the tree's lane, one word:
//   path length (= depth + 1) | pick << 7 | block << 8 | leaf action << 15 | node id of the leaf's parent << 16
SMZ_MASKS_HD inline uint32_t leaf_pack(int b, uint32_t lin, int pick, int action, int A) {
    return (uint32_t)(lin_depth(lin) + 1) | ((uint32_t)pick << 7) | ((uint32_t)b << 8) | ((uint32_t)action << 15) |
           ((uint32_t)owner_node(b, lin, A) << 16);
}
SMZ_MASKS_HD inline int leaf_len(uint32_t w) { return (int)(w & 127u); }
SMZ_MASKS_HD inline int leaf_loc(uint32_t w) { return (int)(((w >> 8) & 127u) << 8 | ((w >> 7) & 1u)); }     // block << 8 | pick
SMZ_MASKS_HD inline int leaf_action(uint32_t w) { return (int)((w >> 15) & 1u); }
SMZ_MASKS_HD inline int leaf_parent(uint32_t w) { return (int)(w >> 16); }

// the lane that holds a tree slot's leaf word: lf = ballot over both passes of "on the path, evaluated, picked child has no
// block" (a lane owns two blocks of ONE tree, and a path ends once: at most one of them).  -1: none.
SMZ_MASKS_HD inline int leaf_lane(uint64_t lf, int tslot) {
    const uint64_t m = lf & tree_lanes(tslot);
    return m ? __builtin_ctzll(m) : -1;
}

}  // namespace smz_masks
