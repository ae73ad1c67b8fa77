// Stand-alone check of stochastic-muzero_amd/csrc/smz_select_masks.hpp (built and run by tests/test_select_masks.py with
// -fsanitize=address,undefined): the mask rule of the block-parallel selection against a plain pointer chase from the root.
//
// A "wave" of 64 emulated lanes holds two trees (tree slot = lane & 1) of up to 64 two-child blocks each; lane l owns blocks
// l >> 1 (pass 0) and 32 + (l >> 1) (pass 1) and keeps their lineage exactly as the kernel does: handed over when the block is
// created, from the lane that owns the parent.  Picks and "evaluated" flags are random; ballots are built from the lanes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "smz_select_masks.hpp"

namespace mk = smz_masks;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
static int rnd_below(int n) { return (int)(rnd() % (uint32_t)n); }

struct Lane {                       // the registers of one lane
    uint32_t lin0 = 0, lin1 = 0;
    uint64_t anc0 = 0, anc1l = 0, anc1h = 0;
};
struct Tree {
    int n = 0;                      // blocks (0 = the slot is switched off)
    int child[64][2];               // block hanging from (block, slot), 0: none
    int parent[64], slot[64], depth[64];
    int pick[64], ok[64], action[64][2];
};
static const int A = 2;
static long n_checked = 0, n_fallback = 0, n_cross = 0, max_len = 0;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// the expansion's hand-off: block e under (pb, ls) at depth d of tree slot t
static void create(Lane *lanes, Tree &T, int t, int e, int pb, int ls) {
    T.child[pb][ls] = e; T.parent[e] = pb; T.slot[e] = ls; T.depth[e] = T.depth[pb] + 1;
    const Lane &pl = lanes[mk::lane_of(pb, t)];
    uint64_t a0, a1;
    mk::anc_child(pb < 32 ? pl.anc0 : pl.anc1l, pb < 32 ? 0 : pl.anc1h, pb, t, a0, a1);
    Lane &el = lanes[mk::lane_of(e, t)];
    const uint32_t lin = mk::lin_pack(T.depth[e], pb, ls);
    if (e < 32) { el.lin0 = lin; el.anc0 = a0; }
    else { el.lin1 = lin; el.anc1l = a0; el.anc1h = a1; }
}
static void reset(Tree &T) {
    T.n = 0;
    for (int b = 0; b < 64; b++) {
        T.child[b][0] = T.child[b][1] = 0; T.parent[b] = T.slot[b] = T.depth[b] = 0; T.pick[b] = 0; T.ok[b] = 1;
        T.action[b][0] = rnd() & 1; T.action[b][1] = rnd() & 1;
    }
}
// shape: 0 random, 1 chain (every block under the previous one)
static void grow(Lane *lanes, Tree &T, int t, int n, int shape) {
    reset(T);
    T.n = n;
    for (int e = 1; e < n; e++) {
        int pb, ls;
        if (shape == 1) { pb = e - 1; ls = rnd() & 1; }
        else do { pb = rnd_below(e); ls = rnd() & 1; } while (T.child[pb][ls] != 0);
        create(lanes, T, t, e, pb, ls);
    }
}
static void roll(Tree &T, int miss_percent, bool follow_chain) {
    for (int b = 0; b < T.n; b++) {
        T.ok[b] = rnd_below(100) >= miss_percent;
        T.pick[b] = rnd() & 1;
        if (follow_chain && b + 1 < T.n) T.pick[b] = T.child[b][1] == b + 1;
        if (!T.ok[b]) T.pick[b] = 0;            // (an unevaluated block leaves a zero word)
    }
}

static void check_wave(Lane *lanes, Tree *trees) {
    // --- the mask rule, lane by lane -------------------------------------------------------------------------------
    uint64_t p0 = 0, p1 = 0, g0 = 0, g1 = 0, fb = 0, lf = 0;
    bool gd0[64], gd1[64], on0[64], on1[64];
    uint32_t mine[64];
    for (int l = 0; l < 64; l++) {
        const Tree &T = trees[l & 1];
        const int b0 = l >> 1, b1 = 32 + (l >> 1);
        if (b0 < T.n && T.pick[b0]) p0 |= (uint64_t)1 << l;
        if (b1 < T.n && T.pick[b1]) p1 |= (uint64_t)1 << l;
    }
    for (int l = 0; l < 64; l++) {
        const Tree &T = trees[l & 1];
        const int b0 = l >> 1, b1 = 32 + (l >> 1), t = l & 1;
        gd0[l] = b0 < T.n && mk::good(b0, lanes[l].lin0, t, p0, p1);
        gd1[l] = b1 < T.n && mk::good(b1, lanes[l].lin1, t, p0, p1);
        if (gd0[l]) g0 |= (uint64_t)1 << l;
        if (gd1[l]) g1 |= (uint64_t)1 << l;
    }
    for (int l = 0; l < 64; l++) {
        const Tree &T = trees[l & 1];
        const int b0 = l >> 1, b1 = 32 + (l >> 1);
        on0[l] = mk::on_path(gd0[l], lanes[l].anc0, 0, g0, g1);
        on1[l] = mk::on_path(gd1[l], lanes[l].anc1l, lanes[l].anc1h, g0, g1);
        const bool ok0 = b0 < T.n && T.ok[b0], ok1 = b1 < T.n && T.ok[b1];
        if ((on0[l] && !ok0) || (on1[l] && !ok1)) fb |= (uint64_t)1 << l;
        const bool lf0 = on0[l] && ok0 && T.child[b0][T.pick[b0]] == 0, lf1 = on1[l] && ok1 && T.child[b1][T.pick[b1]] == 0;
        if (lf0 || lf1) lf |= (uint64_t)1 << l;
        mine[l] = lf0 ? mk::leaf_pack(b0, lanes[l].lin0, T.pick[b0], b0 == 0 ? T.pick[b0] : T.action[b0][T.pick[b0]], A)
                      : mk::leaf_pack(b1, lanes[l].lin1, T.pick[b1], T.action[b1][T.pick[b1]], A);
    }
    // --- against the chase, per tree slot --------------------------------------------------------------------------
    for (int t = 0; t < 2; t++) {
        const Tree &T = trees[t];
        const bool fell = (fb & mk::tree_lanes(t)) != 0;
        if (T.n == 0) {             // a switched-off slot contributes nothing
            CHECK(!fell && mk::leaf_lane(lf, t) < 0 && (g0 & mk::tree_lanes(t)) == 0 && (g1 & mk::tree_lanes(t)) == 0);
            continue;
        }
        std::vector<int> path;      // blocks, root first
        bool missed = false;
        int b = 0;
        for (;;) {
            if (!T.ok[b]) { missed = true; break; }
            path.push_back(b);
            b = T.child[b][T.pick[b]];
            if (b == 0) break;
        }
        n_checked++;
        CHECK(fell == missed);                  // the fallback: exactly when the chase meets an unevaluated block
        if (missed) { n_fallback++; continue; }
        const int len = (int)path.size();
        if (len > max_len) max_len = len;
        // the set of blocks the masks put on the path is the chase's, each at its depth
        std::vector<int> at(64, -1);
        int n_on = 0;
        for (int l = t; l < 64; l += 2) {
            if (on0[l]) { n_on++; CHECK(at[mk::lin_depth(lanes[l].lin0)] < 0); at[mk::lin_depth(lanes[l].lin0)] = l >> 1; }
            if (on1[l]) { n_on++; CHECK(at[mk::lin_depth(lanes[l].lin1)] < 0); at[mk::lin_depth(lanes[l].lin1)] = 32 + (l >> 1); }
        }
        CHECK(n_on == len);
        bool low = false, cross = false;
        for (int d = 0; d < len; d++) {
            CHECK(at[d] == path[d]);
            if (path[d] < 32) low = true; else if (low) cross = true;
        }
        n_cross += cross;
        // the leaf word: length, location, action, parent node
        const int ll = mk::leaf_lane(lf, t);
        CHECK(ll >= 0 && (ll & 1) == t);
        CHECK((lf & mk::tree_lanes(t)) == (uint64_t)1 << ll);          // exactly one lane
        const uint32_t w = mine[ll];
        const int last = path[len - 1], pk = T.pick[last];
        CHECK(mk::leaf_len(w) == len);
        CHECK(mk::leaf_loc(w) == ((last << 8) | pk));
        CHECK(mk::leaf_action(w) == (last == 0 ? pk : T.action[last][pk]));
        // the nodes as the chase names them (select_leaf's node() over the path's last two entries)
        const int leaf_id = last == 0 ? 1 + pk : 1 + A + (last - 1) * 2 + pk;
        int parent_id = 0;
        if (len > 1) { const int pb = path[len - 2], pp = T.pick[pb]; parent_id = pb == 0 ? 1 + pp : 1 + A + (pb - 1) * 2 + pp; }
        CHECK(mk::child_node(last, pk, A) == leaf_id);
        CHECK(mk::leaf_parent(w) == parent_id);
    }
}

int main() {
    Lane lanes[64];
    Tree trees[2];
    auto fresh = [&] { for (auto &l : lanes) l = Lane(); reset(trees[0]); reset(trees[1]); };
    // random trees, both tree slots interleaved in the ballots, grown block by block with a check after every expansion round
    for (int rep = 0; rep < 6000; rep++) {
        fresh();
        const int n0 = 1 + rnd_below(64), n1 = rep % 7 == 0 ? 0 : 1 + rnd_below(64);
        grow(lanes, trees[0], 0, n0, rep % 5 == 0);
        if (n1) grow(lanes, trees[1], 1, n1, rep % 3 == 0);
        for (int k = 0; k < 4; k++) {
            const int miss = k == 0 ? 0 : (k == 1 ? 3 : (k == 2 ? 15 : 50));
            roll(trees[0], miss, rep % 5 == 0 && k < 2);
            roll(trees[1], miss, rep % 3 == 0 && k < 2);
            check_wave(lanes, trees);
        }
    }
    const long cross_random = n_cross;
    // a single root in one slot, the other switched off -- and the other way round
    for (int t = 0; t < 2; t++) {
        fresh();
        grow(lanes, trees[t], t, 1, 0);
        for (int k = 0; k < 4; k++) { roll(trees[t], 0, false); check_wave(lanes, trees); }
        roll(trees[t], 100, false); check_wave(lanes, trees);
    }
    // a 51-deep chain followed to its end (the path crosses from blocks below 32 into blocks from 32 on), next to a 64-block one
    fresh();
    grow(lanes, trees[0], 0, 51, 1);
    grow(lanes, trees[1], 1, 64, 1);
    roll(trees[0], 0, true); roll(trees[1], 0, true);
    const long before = n_cross;
    check_wave(lanes, trees);
    CHECK(max_len == 64 && n_cross == before + 2);
    // the same chains with one unevaluated block each
    trees[0].ok[40] = 0; trees[0].pick[40] = 0; trees[1].ok[0] = 0; trees[1].pick[0] = 0;
    const long fb_before = n_fallback;
    check_wave(lanes, trees);
    CHECK(n_fallback == fb_before + 2);
    // (blocks are created in index order, so a path never returns from the second pass to the first)
    CHECK(cross_random > 100 && n_fallback > 1000 && n_checked - n_fallback > 10000);
    std::printf("ok: %ld descents checked, %ld of them fallbacks, %ld crossing into the second pass, longest path %ld\n", n_checked,
                n_fallback, n_cross, max_len);
    return 0;
}
