// smz_othello.hpp -- the rules of Othello (Reversi), one body for the host and the device (C ABI: smz_othello_*,
// csrc/smz_envothello.hip).
//
// Othello is the engine's large-action game: 8 x 8 squares, two colours, 65 actions (place a disc on square 0 .. 63, or pass:
// 64), colour 0 first.  Everything here is integer arithmetic on two 64-bit registers and the colour to move, so the device
// env, the host functions and a restatement in any other language agree bit for bit.
//
// Position: TWO 64-bit words, word p = the discs of colour p.  Bit 8 * r + c is row r, column c (the observation index too).
// The side to move is part of the state: a pass changes it and nothing else, so it cannot be read off the board.
//
// Moves and flips are shift-and-mask fills over the 8 directions.  A direction is a shift by +-1, +-7, +-8, +-9 bits; for the
// six with a horizontal component the opponent's discs a run may pass through are masked to the files b .. g, so no run
// continues from the h-file of one row into the a-file of the next (a run that reaches the a- or h-file ends there: the edge
// square itself can only be the mover's closing disc or the square played).  A run is at most 6 opponent discs long: one
// seed step and five fill steps.  Every shift count is a template argument; nothing is indexed with a run-time value.
//
// No HIP types: hipcc compiles it for both sides, a plain C++ compiler for the host alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SMZ_OTH_HD __host__ __device__
#else
#define SMZ_OTH_HD
#endif

namespace smzoth {

constexpr int kSquares = 64, kPass = 64, kActions = 65, kObs = 65;
constexpr uint64_t kInner = 0x7E7E7E7E7E7E7E7Eull;             // the files b .. g
constexpr uint64_t kStart0 = (1ull << 28) | (1ull << 35);      // colour 0 on (3,4) and (4,3)
constexpr uint64_t kStart1 = (1ull << 27) | (1ull << 36);      // colour 1 on (3,3) and (4,4)

SMZ_OTH_HD inline int popcount(uint64_t x) { return __builtin_popcountll(x); }

// One step in direction S (bits): S > 0 towards higher squares.
template <int S>
SMZ_OTH_HD inline uint64_t shift(uint64_t x) {
    if constexpr (S > 0) return x << S;
    else return x >> (-S);
}

// The opponent discs a run in direction S may pass through.
template <int S>
SMZ_OTH_HD inline uint64_t passable(uint64_t opp) {
    if constexpr (S == 8 || S == -8) return opp;
    else return opp & kInner;
}

// The run of opponent discs that starts next to `from` (one or more squares) in direction S.
template <int S>
SMZ_OTH_HD inline uint64_t run(uint64_t from, uint64_t opp) {
    const uint64_t m = passable<S>(opp);
    uint64_t t = m & shift<S>(from);
    t |= m & shift<S>(t);
    t |= m & shift<S>(t);
    t |= m & shift<S>(t);
    t |= m & shift<S>(t);
    t |= m & shift<S>(t);
    return t;
}

// The squares just past a run that starts at a disc of `me`, in direction S (not yet masked to the empty squares).
template <int S>
SMZ_OTH_HD inline uint64_t moves_dir(uint64_t me, uint64_t opp) { return shift<S>(run<S>(me, opp)); }

// The squares on which the colour with discs `me` may place a disc.
SMZ_OTH_HD inline uint64_t moves(uint64_t me, uint64_t opp) {
    const uint64_t m = moves_dir<1>(me, opp) | moves_dir<-1>(me, opp) | moves_dir<8>(me, opp) | moves_dir<-8>(me, opp) |
                       moves_dir<9>(me, opp) | moves_dir<-9>(me, opp) | moves_dir<7>(me, opp) | moves_dir<-7>(me, opp);
    return m & ~(me | opp);
}

// The opponent discs that a disc placed on `x` (one bit) turns in direction S: the run from x, when a disc of `me` ends it.
template <int S>
SMZ_OTH_HD inline uint64_t flips_dir(uint64_t x, uint64_t me, uint64_t opp) {
    const uint64_t t = run<S>(x, opp);
    return (shift<S>(t) & me) != 0 ? t : 0ull;               // (shift(t) is t's tail and the square past it; t holds no disc of me)
}

SMZ_OTH_HD inline uint64_t flips(uint64_t x, uint64_t me, uint64_t opp) {
    return flips_dir<1>(x, me, opp) | flips_dir<-1>(x, me, opp) | flips_dir<8>(x, me, opp) | flips_dir<-8>(x, me, opp) |
           flips_dir<9>(x, me, opp) | flips_dir<-9>(x, me, opp) | flips_dir<7>(x, me, opp) | flips_dir<-7>(x, me, opp);
}

// The bit of square `sq` in 0 .. 63, from constant shifts: one conditional doubling of the distance per bit of sq.
SMZ_OTH_HD inline uint64_t square_bit(int sq) {
    uint64_t x = 1ull;
    x = (sq & 1) ? x << 1 : x;
    x = (sq & 2) ? x << 2 : x;
    x = (sq & 4) ? x << 4 : x;
    x = (sq & 8) ? x << 8 : x;
    x = (sq & 16) ? x << 16 : x;
    x = (sq & 32) ? x << 32 : x;
    return x;
}

// A position no move can be made on: neither colour has a placement (a full board and a wipe-out are cases of it).
SMZ_OTH_HD inline bool finished(uint64_t d0, uint64_t d1) { return (moves(d0, d1) | moves(d1, d0)) == 0; }

// The move `action` of colour `mover`.  Returns whether it was legal; an illegal one changes nothing.  `over`: the position as
// it is after the call is finished; `reward`: 0 but for the move that ends the game, which gets +1 / -1 / 0 as the colour that
// made it has more / fewer / as many discs as the other.
SMZ_OTH_HD inline bool play(uint64_t &d0, uint64_t &d1, int &mover, int action, float &reward, bool &over) {
    const bool second = mover != 0;
    const uint64_t me = second ? d1 : d0, opp = second ? d0 : d1;
    const uint64_t mine = moves(me, opp), theirs = moves(opp, me);
    reward = 0.0f;
    over = (mine | theirs) == 0;
    if (over || action < 0 || action > kPass) return false;
    if (action == kPass) {
        if (mine != 0) return false;                         // (theirs != 0: the position is not finished)
        mover ^= 1;
        return true;
    }
    const uint64_t x = square_bit(action);
    if ((x & mine) == 0) return false;
    const uint64_t f = flips(x, me, opp);
    const uint64_t me2 = me | x | f, opp2 = opp & ~f;
    d0 = second ? opp2 : me2;
    d1 = second ? me2 : opp2;
    mover ^= 1;
    over = (moves(me2, opp2) | moves(opp2, me2)) == 0;
    if (over) {
        const int a = popcount(me2), b = popcount(opp2);
        reward = a > b ? 1.0f : (a < b ? -1.0f : 0.0f);
    }
    return true;
}

// obs[8 * r + c] for the constant square i = 8 * r + c: +1 a colour-0 disc, -1 a colour-1 disc, 0 empty
template <int I>
SMZ_OTH_HD inline float cell_obs(uint64_t d0, uint64_t d1) {
    return (float)((int)((d0 >> I) & 1ull) - (int)((d1 >> I) & 1ull));
}
// obs[64]: +1 when colour 0 is to move, else -1
SMZ_OTH_HD inline float mover_obs(int mover) { return mover ? -1.0f : 1.0f; }

template <typename T, int I>
SMZ_OTH_HD inline void write_cells(T *row, uint64_t d0, uint64_t d1) {
    if constexpr (I < kSquares) {
        row[I] = (T)cell_obs<I>(d0, d1);
        write_cells<T, I + 1>(row, d0, d1);
    }
}
// The 65 observations of a position, float or double.
template <typename T>
SMZ_OTH_HD inline void write_obs(T *row, uint64_t d0, uint64_t d1, int mover) {
    write_cells<T, 0>(row, d0, d1);
    row[kSquares] = (T)mover_obs(mover);
}

}  // namespace smzoth
