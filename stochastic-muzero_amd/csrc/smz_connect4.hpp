// smz_connect4.hpp -- the rules of Connect Four, one body for the host and the device (C ABI: smz_connect4_*,
// csrc/smz_envconnect4.hip).
//
// Connect Four is the engine's two-player game: 6 rows x 7 columns, seven actions (drop a disc into column 0 .. 6), two
// colours that move in turn, colour 0 first.  Everything here is integer arithmetic on two 64-bit registers, so the device
// env, the host functions and a restatement in any other language agree bit for bit.
//
// Position: TWO 64-bit words, word p = the discs of colour p.  Bit 7 * c + r is column c, row r, r = 0 the bottom row.  Bit 6
// of every column's 7-bit group is a sentinel that is never set: a shifted copy of the board cannot carry a line from the top
// of one column into the bottom of the next.  Bits 49 .. 63 are never set either.
//
// Side to move: read off the board, colour popcount(discs[0] | discs[1]) & 1.  Height of column c: popcount((all >> 7c) & 0x3f)
// (discs fall, so a column's discs are its low bits).  A move is illegal when the column is full, when the action is outside
// 0 .. 6 and on a finished board (one that already holds a line of four or 42 discs).  A move wins when it gives the mover
// four in a row: m = b & (b >> s); m & (m >> 2s) for s = 1 (vertical), 7 (horizontal), 6 and 8 (the diagonals).
//
// No HIP types: hipcc compiles it for both sides, a plain C++ compiler for the host alone.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SMZ_C4_HD __host__ __device__
#else
#define SMZ_C4_HD
#endif

namespace smzc4 {

constexpr int kRows = 6, kCols = 7, kCells = kRows * kCols;

SMZ_C4_HD inline int popcount(uint64_t x) { return __builtin_popcountll(x); }

// Does `b` (the discs of ONE colour) hold four in a row?
SMZ_C4_HD inline bool has_line(uint64_t b) {
    uint64_t hit = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = k == 0 ? 1 : k == 1 ? 7 : k == 2 ? 6 : 8;
        const uint64_t m = b & (b >> s);
        hit |= m & (m >> (2 * s));
    }
    return hit != 0;
}

// A board no move can be made on: a line of either colour, or all 42 cells taken.
SMZ_C4_HD inline bool finished(uint64_t d0, uint64_t d1) {
    return has_line(d0) || has_line(d1) || popcount(d0 | d1) == kCells;
}

// Colour of the side to move: 0 on the empty board.
SMZ_C4_HD inline int to_move(uint64_t d0, uint64_t d1) { return popcount(d0 | d1) & 1; }

// The move `action` of the side to move.  Returns whether it was legal; an illegal one changes nothing.  `won`: the move made
// four in a row; `over`: the board as it is after the call is finished.
SMZ_C4_HD inline bool play(uint64_t &d0, uint64_t &d1, int action, bool &won, bool &over) {
    const uint64_t all = d0 | d1;
    won = false;
    over = finished(d0, d1);
    if (over || action < 0 || action >= kCols) return false;
    const int height = popcount((all >> (7 * action)) & 0x3full);
    if (height >= kRows) return false;
    const uint64_t bit = 1ull << (7 * action + height);
    const bool second = (popcount(all) & 1) != 0;
    const uint64_t mine = (second ? d1 : d0) | bit;
    d0 = second ? d0 : mine;
    d1 = second ? mine : d1;
    won = has_line(mine);
    over = won || popcount(all) + 1 == kCells;
    return true;
}

// obs[7 * r + c], r = 0 the bottom row: +1 a colour-0 disc, -1 a colour-1 disc, 0 empty
SMZ_C4_HD inline float cell_obs(uint64_t d0, uint64_t d1, int r, int c) {
    const int bit = 7 * c + r;
    return (float)((int)((d0 >> bit) & 1ull) - (int)((d1 >> bit) & 1ull));
}
// obs[42]: +1 when colour 0 is to move, else -1
SMZ_C4_HD inline float mover_obs(uint64_t d0, uint64_t d1) { return to_move(d0, d1) ? -1.0f : 1.0f; }

}  // namespace smzc4
