"""A plain-Python restatement of the Othello rules of include/smz.h (smz_othello_step_ctl), shared by the Othello tests: an
8 x 8 list of cells, rays walked square by square, no bitboards.  It imports neither host_envs.OthelloBatch nor the C core."""
import math

import numpy as np

N, OBS, A, PASS, F = 8, 65, 65, 64, 263
DIRS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def empty():
    return [[None] * N for _ in range(N)]                   # cells[r][c]: None | 0 | 1


def start():
    cells = empty()
    cells[3][4] = cells[4][3] = 0
    cells[3][3] = cells[4][4] = 1
    return cells


def count(cells, colour=None):
    return sum((v is not None) if colour is None else (v == colour) for row in cells for v in row)


def ray_flips(cells, r, c, dr, dc, colour):
    """The opponent cells turned along one ray by a disc of `colour` on (r, c): a contiguous run ended by a disc of `colour`."""
    run = []
    r, c = r + dr, c + dc
    while 0 <= r < N and 0 <= c < N and cells[r][c] == 1 - colour:
        run.append((r, c))
        r, c = r + dr, c + dc
    if run and 0 <= r < N and 0 <= c < N and cells[r][c] == colour:
        return run
    return []


def flips(cells, r, c, colour):
    out = []
    for dr, dc in DIRS:
        if 0 <= r + dr < N and 0 <= c + dc < N and cells[r + dr][c + dc] == 1 - colour:     # (else the ray's run is empty)
            out += ray_flips(cells, r, c, dr, dc, colour)
    return out


def placements(cells, colour):
    """The squares (8 * r + c) on which `colour` may place a disc."""
    return [N * r + c for r in range(N) for c in range(N) if cells[r][c] is None and flips(cells, r, c, colour)]


def finished(cells):
    return not placements(cells, 0) and not placements(cells, 1)


def legal_actions(cells, mover, both=None):
    """The legal actions of `mover`; both: (placements of colour 0, of colour 1) when the caller has them already."""
    mine, theirs = (placements(cells, mover), placements(cells, 1 - mover)) if both is None else (both[mover], both[1 - mover])
    if not mine and not theirs:
        return []
    return mine or [PASS]                                   # (not finished and no placement: the opponent has one)


def mask(cells, colour):
    return sum(1 << sq for sq in placements(cells, colour))


def step(cells, mover, action, both=None):
    """-> (cells, mover, reward, terminated, illegal); an illegal move returns the cells and the mover it was given.  both: as
    for legal_actions."""
    if both is None:
        both = (placements(cells, 0), placements(cells, 1))
    if action not in legal_actions(cells, mover, both):
        return cells, mover, 0.0, not both[0] and not both[1], True
    if action == PASS:
        return cells, 1 - mover, 0.0, False, False
    r, c = divmod(action, N)
    new = [list(row) for row in cells]
    new[r][c] = mover
    for fr, fc in flips(cells, r, c, mover):
        new[fr][fc] = mover
    over = finished(new)
    mine, other = count(new, mover), count(new, 1 - mover)
    return new, 1 - mover, float((mine > other) - (mine < other)) if over else 0.0, over, False


def obs(cells, mover):
    o = [0.0 if cells[r][c] is None else (1.0, -1.0)[cells[r][c]] for r in range(N) for c in range(N)]
    return np.array(o + [-1.0 if mover else 1.0], np.float32)


def words(cells):
    d = [0, 0]
    for r in range(N):
        for c in range(N):
            if cells[r][c] is not None:
                d[cells[r][c]] |= 1 << (N * r + c)
    return d


def from_rows(rows):
    """cells from 8 strings: 'x' colour 0, 'o' colour 1, '.' empty."""
    assert len(rows) == N and all(len(r) == N for r in rows)
    return [[{"x": 0, "o": 1, ".": None}[ch] for ch in row] for row in rows]


def illegal_reward(steps_so_far, limit):
    return float(min(-steps_so_far, -limit if limit > 0 else -math.inf, -1))


# ---- crafted positions: (cells, mover, action) ----------------------------------------------------------------------------
def all_directions():
    """Colour 0 on (3,3) flips a run in every one of the 8 directions (lengths 1 .. 3, each ended by its own disc)."""
    return from_rows(["x..x..x.",
                      ".o.o.o..",
                      "..ooo...",
                      "xoo.ooox",
                      "..ooo...",
                      ".o.o.o..",
                      "x..o..x.",
                      "...x...."]), 0, 27


def wipe_out(colour=0):
    """`colour` takes the other colour's last disc: the game ends with 3 discs on the board."""
    row = "..xo...." if colour == 0 else "..ox...."
    return from_rows(["........"] * 3 + [row] + ["........"] * 4), colour, 28


ELSEWHERE = "xo......"                                      # (colour 0 may play (r, 2): the position is not finished)


def edge_runs():
    """Runs that reach the a- and h-files in each horizontal and diagonal direction: (cells, mover, action, legal).  The legal
    ones flip six discs up to the file; the refused ones have a run that stops AT the file and a disc of the mover on the
    square a shift would wrap to (the next or the previous row's far file), so rules that wrapped would accept them."""
    e, out = "........", []
    out.append((from_rows([e, e, e, ".oooooox", "ox......", e, e, e]), 0, 24, True))           # east, closed on the h-file
    out.append((from_rows([e, e, ".......x", "xoooooo.", e, e, e, e]), 0, 31, True))           # west, closed on the a-file
    out.append((from_rows([e, e, e, "x....ooo", "x.......", e, e, ELSEWHERE]), 0, 28, False))  # east: bit 31 + 1 = (4,0)
    out.append((from_rows([e, e, ".......x", "ooo....x", e, e, e, ELSEWHERE]), 0, 27, False))  # west: bit 24 - 1 = (2,7)
    down = from_rows([e, ".o....o.", "..o..o..", "...oo...", "...oo...", "..o..o..", ".o....o.", "x......x"])
    out += [(down, 0, 0, True), (down, 0, 7, True)]                                            # south-east, south-west
    up = from_rows(["x......x", ".o....o.", "..o..o..", "...oo...", "...oo...", "..o..o..", ".o....o.", e])
    out += [(up, 0, 56, True), (up, 0, 63, True)]                                              # north-east, north-west
    out.append((from_rows([e, ".....o..", "......o.", ".......o", e, "x.......", e, ELSEWHERE]), 0, 4, False))   # 31 + 9 = (5,0)
    out.append((from_rows([e, "..o.....", ".o......", "o......x", e, e, e, ELSEWHERE]), 0, 3, False))           # 24 + 7 = (3,7)
    out.append((from_rows([ELSEWHERE, e, ".......x", e, "o.......", ".o......", "..o.....", e]), 0, 59, False))  # 32 - 9 = (2,7)
    out.append((from_rows([ELSEWHERE, e, e, e, "x......o", "......o.", ".....o..", e]), 0, 60, False))          # 39 - 7 = (4,0)
    return out


def refused_pass():
    return start(), 0, PASS


def legal_pass():
    """Colour 1 has no placement and colour 0 has one: colour 1 passes (and colour 0's (0,2) then takes the last disc)."""
    return from_rows(["xo......"] + ["........"] * 7), 1, PASS


def finished_position():
    """Two discs that see no run: nobody can move."""
    return from_rows(["x......o"] + ["........"] * 7), 0
