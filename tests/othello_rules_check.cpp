// othello_rules_check.cpp -- csrc/smz_othello.hpp under a plain host compiler (tests/test_othello_rules_sanitized.py builds it
// with -fsanitize=address,undefined): random legal games with the invariants of the rules checked at every move.
//   * the colours' words are disjoint;
//   * the move mask is a subset of the empty squares, for both colours;
//   * the flips of a placement are a non-empty subset of the opponent's discs;
//   * a placement adds exactly one disc to the board, a pass none, and both change the mover;
//   * an action that is not legal changes nothing;
//   * `over` says that neither colour has a placement, and only the move that ends a game has a reward.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "smz_othello.hpp"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {                                        // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            std::printf("FAILED %s (line %d): game %d move %d d0 %016llx d1 %016llx mover %d action %d\n", #cond, __LINE__, game, \
                        move, (unsigned long long)d0, (unsigned long long)d1, mover, action);                \
            return 1;                                                                                        \
        }                                                                                                    \
    } while (0)

}  // namespace

int main() {
    using namespace smzoth;
    long long moves_played = 0, passes = 0, refused = 0, early = 0;
    for (int game = 0; game < 3000; game++) {
        uint64_t d0 = kStart0, d1 = kStart1;
        int mover = 0, move = 0, action = -1;
        for (;; move++) {
            CHECK((d0 & d1) == 0);
            const uint64_t me = mover ? d1 : d0, opp = mover ? d0 : d1, empty = ~(d0 | d1);
            const uint64_t mine = moves(me, opp), theirs = moves(opp, me);
            CHECK((mine & ~empty) == 0 && (theirs & ~empty) == 0);
            CHECK(finished(d0, d1) == ((mine | theirs) == 0));
            float reward = 7.f;
            bool over = false;
            // an action that is not legal: a square outside the mask, a pass while a placement exists, out of range
            {
                action = (int)(next_u64() % 69) - 2;
                const bool legal_here = (mine | theirs) != 0 && ((action >= 0 && action < 64 && ((mine >> action) & 1ull)) ||
                                                                 (action == kPass && mine == 0));
                if (!legal_here) {
                    uint64_t a0 = d0, a1 = d1;
                    int m = mover;
                    CHECK(!play(a0, a1, m, action, reward, over));
                    CHECK(a0 == d0 && a1 == d1 && m == mover && reward == 0.f && over == ((mine | theirs) == 0));
                    refused++;
                }
            }
            if ((mine | theirs) == 0) break;
            const int discs_before = popcount(d0 | d1);
            if (mine == 0) {
                action = kPass;
                uint64_t a0 = d0, a1 = d1;
                int m = mover;
                CHECK(play(a0, a1, m, action, reward, over));
                CHECK(a0 == d0 && a1 == d1 && m == (mover ^ 1) && reward == 0.f && !over);
                mover = m;
                passes++;
                continue;
            }
            int pick = (int)(next_u64() % (uint64_t)popcount(mine));
            action = 0;
            for (int sq = 0; sq < 64; sq++)
                if ((mine >> sq) & 1ull) {
                    if (pick == 0) action = sq;
                    pick--;
                }
            const uint64_t x = square_bit(action);
            CHECK(x == (1ull << action));
            const uint64_t f = flips(x, me, opp);
            CHECK(f != 0 && (f & ~opp) == 0);
            uint64_t a0 = d0, a1 = d1;
            int m = mover;
            CHECK(play(a0, a1, m, action, reward, over));
            CHECK((a0 & a1) == 0 && m == (mover ^ 1));
            CHECK(popcount(a0 | a1) == discs_before + 1);
            CHECK((mover ? a1 : a0) == (me | x | f) && (mover ? a0 : a1) == (opp & ~f));
            CHECK(over == finished(a0, a1));
            const int mine_n = popcount(mover ? a1 : a0), their_n = popcount(mover ? a0 : a1);
            CHECK(reward == (over ? (mine_n > their_n ? 1.f : mine_n < their_n ? -1.f : 0.f) : 0.f));
            d0 = a0;
            d1 = a1;
            mover = m;
            moves_played++;
        }
        early += popcount(d0 | d1) < 64;
        // the observations of the final position: every cell in {-1, 0, +1} and equal to the discs
        float row[kObs];
        write_obs(row, d0, d1, mover);
        for (int sq = 0; sq < 64; sq++) {
            action = sq;
            CHECK(row[sq] == (float)((int)((d0 >> sq) & 1ull) - (int)((d1 >> sq) & 1ull)));
        }
        CHECK(row[64] == (mover ? -1.f : 1.f));
    }
    if (passes == 0 || early == 0 || refused == 0) {
        std::printf("FAILED coverage: passes %lld early ends %lld refused %lld\n", passes, early, refused);
        return 1;
    }
    std::printf("ok: 3000 games, %lld placements, %lld passes, %lld refused actions, %lld games ended before 64 discs\n",
                moves_played, passes, refused, early);
    return 0;
}
