// smz_2048.hpp -- the rules of 2048, one body for the host and the device (C ABI: smz_2048_*, csrc/smz_env2048.hip).
//
// 2048 is the single-player stochastic game of the Stochastic MuZero paper: four actions, a chance event (the tile spawn)
// after every move, and moves that are illegal.  Everything here is integer arithmetic on registers, so the device env, the
// host functions and a restatement in any other language agree bit for bit.
//
// Board: 16 exponents in row-major order, 0 = empty, k = the tile 2^k.  A board is handled as FOUR 32-bit words, one per
// row, cell (r, c) in byte c of word r -- the 16 bytes of the uint8 [16] array as a little-endian machine loads them, so the
// kernel moves a board with one 128-bit access and never indexes an array with a run-time value (no scratch memory).
// Exponents are whole bytes, not nibbles: 15 + 15 -> 16 works.  Domain: exponents <= 30 (a merge's value must fit the 32-bit
// reward sum; the largest tile a 4 x 4 board can hold is 2^17).
//
// Actions: 0 up, 1 right, 2 down, 3 left.  A move slides every line towards the action's edge; each tile merges at most
// once per move and merges resolve from that edge: [2,2,2,2] -> [4,4,0,0], [2,2,4,0] -> [4,4,0,0], [4,2,2,0] -> [4,4,0,0].
// The reward of a move is the sum of the values of the tiles its merges created.  A move that leaves the board unchanged is
// illegal.  After a legal move one tile spawns: with m empty cells, in row-major order, cell number (int)floor(u0 * m) gets
// exponent 2 when u1 < 0.1, else 1 (u0, u1 in [0, 1): two draws of the caller's generator).  A game is over when, after the
// spawn, no action is legal.
//
// No HIP types: hipcc compiles it for both sides, a plain C++ compiler for the host alone.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SMZ_2048_HD __host__ __device__
#else
#define SMZ_2048_HD
#endif

namespace smz2048 {

// One line, byte 0 = the cell at the edge the tiles move towards.  `gain` receives the values of the merged tiles.
SMZ_2048_HD inline uint32_t slide_line(uint32_t line, uint32_t &gain) {
    uint32_t out = 0, last = 0;      // last: the tile in byte p - 1 of `out` while it may still merge (0: it may not)
    int p = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t v = (line >> (8 * j)) & 255u;
        if (!v) continue;
        if (v == last) {
            out += 1u << (8 * (p - 1));                  // byte p - 1: v -> v + 1
            gain += 1u << ((v + 1) & 31u);
            last = 0;
        } else {
            out |= v << (8 * p);
            p++;
            last = v;
        }
    }
    return out;
}

SMZ_2048_HD inline uint32_t reverse_line(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}

SMZ_2048_HD inline void transpose(uint32_t w[4]) {
    uint32_t t[4];
#pragma unroll
    for (int c = 0; c < 4; c++)
        t[c] = ((w[0] >> (8 * c)) & 255u) | (((w[1] >> (8 * c)) & 255u) << 8) | (((w[2] >> (8 * c)) & 255u) << 16) |
               (((w[3] >> (8 * c)) & 255u) << 24);
#pragma unroll
    for (int c = 0; c < 4; c++) w[c] = t[c];
}

// The slide of `action` (0 .. 3; anything else is the caller's to refuse).  Returns whether the board changed, i.e. whether the
// move is legal; an illegal move leaves w and gain as they were.
SMZ_2048_HD inline bool move(uint32_t w[4], int action, uint32_t &gain) {
    const bool column = (action & 1) == 0;               // up / down: the lines are the columns
    const bool far_edge = action == 1 || action == 2;    // right / down: the lines run from the far end
    uint32_t n[4] = {w[0], w[1], w[2], w[3]};
    uint32_t g = 0;
    if (column) transpose(n);
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const uint32_t line = far_edge ? reverse_line(n[l]) : n[l];
        const uint32_t out = slide_line(line, g);
        n[l] = far_edge ? reverse_line(out) : out;
    }
    if (column) transpose(n);
    const bool changed = n[0] != w[0] || n[1] != w[1] || n[2] != w[2] || n[3] != w[3];
    if (changed) {
#pragma unroll
        for (int r = 0; r < 4; r++) w[r] = n[r];
        gain += g;
    }
    return changed;
}

SMZ_2048_HD inline int empty_cells(const uint32_t w[4]) {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) m += ((w[i >> 2] >> (8 * (i & 3))) & 255u) == 0 ? 1 : 0;
    return m;
}

// Is any action legal?  A board with tiles and room always has a tile next to an empty cell; a full board needs two equal
// neighbours; an empty board has nothing to move.
SMZ_2048_HD inline bool any_legal(const uint32_t w[4]) {
    const int m = empty_cells(w);
    if (m == 16) return false;
    if (m > 0) return true;
    bool eq = false;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t h = w[r] ^ (w[r] >> 8);           // bytes 0 .. 2: a cell against its right neighbour
        eq = eq || (h & 0xFFu) == 0 || (h & 0xFF00u) == 0 || (h & 0xFF0000u) == 0;
        if (r < 3) {
            const uint32_t v = w[r] ^ w[r + 1];          // a cell against the one below
            eq = eq || (v & 0xFFu) == 0 || (v & 0xFF00u) == 0 || (v & 0xFF0000u) == 0 || (v & 0xFF000000u) == 0;
        }
    }
    return eq;
}

// The chance event: one tile into empty cell number floor(u0 * m) of the m empty cells (row-major); nothing on a full board.
SMZ_2048_HD inline void spawn(uint32_t w[4], double u0, double u1) {
    const int m = empty_cells(w);
    if (m == 0) return;
    const int k = (int)floor(u0 * (double)m);
    const uint32_t e = u1 < 0.1 ? 2u : 1u;
    int seen = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (((w[i >> 2] >> (8 * (i & 3))) & 255u) == 0) {
            if (seen == k) w[i >> 2] |= e << (8 * (i & 3));
            seen++;
        }
    }
}

// uint8 [16] <-> row words, whatever the byte order of the machine
SMZ_2048_HD inline void load(const uint8_t b[16], uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 4; r++)
        w[r] = (uint32_t)b[4 * r] | ((uint32_t)b[4 * r + 1] << 8) | ((uint32_t)b[4 * r + 2] << 16) | ((uint32_t)b[4 * r + 3] << 24);
}
SMZ_2048_HD inline void store(const uint32_t w[4], uint8_t b[16]) {
#pragma unroll
    for (int i = 0; i < 16; i++) b[i] = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 255u);
}

}  // namespace smz2048
