"""The rules of the Connect Four environment on the CPU: the C rule core compiled for the host (smz_connect4_host_step),
host_envs.HostConnect4 and host_envs.Connect4Batch against a plain-Python restatement written here from the rules as
include/smz.h states them: a 6 x 7 list of cells and a scan of all 69 lines of four, no bitboards (it imports neither
Connect4Batch nor the C core).  Integer rules and exact float32 observations: every comparison is bit for bit."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


# ---- the restatement ------------------------------------------------------------------------------------------------------
ROWS, COLS = 6, 7
DIRECTIONS = {"horizontal": (0, 1), "vertical": (1, 0), "rising": (1, 1), "falling": (-1, 1)}     # (rows, columns) per step
LINES = [(name, [(r + i * dr, c + i * dc) for i in range(4)])
         for name, (dr, dc) in DIRECTIONS.items() for r in range(ROWS) for c in range(COLS)
         if 0 <= r + 3 * dr < ROWS and 0 <= c + 3 * dc < COLS]
assert len(LINES) == 69


def ref_empty():
    return [[None] * COLS for _ in range(ROWS)]         # cells[r][c], r = 0 the bottom row; None | 0 | 1


def ref_count(cells):
    return sum(v is not None for row in cells for v in row)


def ref_lines_of(cells, colour):
    return [(name, line) for name, line in LINES if all(cells[r][c] == colour for r, c in line)]


def ref_finished(cells):
    return bool(ref_lines_of(cells, 0)) or bool(ref_lines_of(cells, 1)) or ref_count(cells) == ROWS * COLS


def ref_height(cells, c):
    return sum(cells[r][c] is not None for r in range(ROWS))


def ref_step(cells, action):
    """-> (cells, reward, terminated, illegal); an illegal move returns the cells it was given."""
    if action not in range(COLS) or ref_finished(cells) or ref_height(cells, action) == ROWS:
        return cells, 0.0, ref_finished(cells), True
    colour = ref_count(cells) % 2
    new = [list(row) for row in cells]
    new[ref_height(cells, action)][action] = colour
    won = bool(ref_lines_of(new, colour))
    return new, 1.0 if won else 0.0, won or ref_count(new) == ROWS * COLS, False


def ref_obs(cells):
    obs = [0.0 if cells[r][c] is None else (1.0, -1.0)[cells[r][c]] for r in range(ROWS) for c in range(COLS)]
    return np.array(obs + [1.0 if ref_count(cells) % 2 == 0 else -1.0], np.float32)


def words(cells):
    """The two uint64 words of a position: bit 7 * c + r of word p is a colour-p disc in column c, row r."""
    d = [0, 0]
    for r in range(ROWS):
        for c in range(COLS):
            if cells[r][c] is not None:
                d[cells[r][c]] |= 1 << (7 * c + r)
    return d


# ---- the implementations --------------------------------------------------------------------------------------------------
def c_step(lib, d, action):
    w = (C.c_uint64 * 2)(*d)
    r, term, ill = C.c_float(-7.0), C.c_int(-7), C.c_int(-7)
    assert lib.smz_connect4_host_step(w, action, C.byref(r), C.byref(term), C.byref(ill)) == 0
    return list(w), r.value, bool(term.value), bool(ill.value)


def everywhere(cells, action):
    """One move on one position through the C core, HostConnect4 and Connect4Batch, each against the restatement, whose result
    it returns."""
    lib, he = _pkg("_lib").load(), _pkg("host_envs")
    new, reward, term, illegal = ref_step(cells, action)
    d, w = words(cells), words(new)
    assert c_step(lib, d, action) == (w, reward, term, illegal)
    assert lib.smz_connect4_host_step((C.c_uint64 * 2)(*d), action, None, None, None) == 0          # outputs may be NULL
    single = he.HostConnect4()
    single.reset(seed=5)
    single.discs[:] = d
    if illegal:
        with pytest.raises(ValueError):
            single.step(action)
    else:
        o, r, t, trunc, _ = single.step(action)
        assert (r, t, trunc) == (reward, term, False)
        assert o.dtype == np.float32 and np.array_equal(o, ref_obs(new))
    assert [int(x) for x in single.discs] == w
    envs = [he.HostConnect4() for _ in range(3)]                    # the move in the middle row of a slice; the others stand still
    batch = he.HostConnect4.make_batch(envs)
    assert isinstance(batch, he.Connect4Batch) and batch.discs.dtype == np.uint64
    batch.discs[1] = d
    obs, r, t, ill = batch.step_batch(np.array([3, action, 3]), np.array([False, True, False]))
    assert (float(r[1]), bool(t[1]), bool(ill[1])) == (reward, term, illegal)
    assert obs.dtype == np.float32 and np.array_equal(obs[1], ref_obs(new)) and np.array_equal(obs[0], ref_obs(ref_empty()))
    assert batch.discs.tolist() == [[0, 0], w, [0, 0]] and [int(x) for x in envs[1].discs] == w and not ill[0] and not ill[2]
    return new, reward, term, illegal


# ---- crafted boards -------------------------------------------------------------------------------------------------------
def filler(r, c, shift=0):
    """A pattern without any line of four, whatever part of the board it covers (with either shift)."""
    return (r // 2 + c + shift) & 1


def craft(discs, last, colour, wins):
    """A position in which `colour` is to move and the cells `discs` hold its discs, but for `last`, the cell its next move
    (column last[1]) takes.  Whatever lies under those cells is filler (the shift of the two with which the position has no
    line yet and, where the move is not meant to win, the filler adds none to it); one more disc of the other colour, on top of the column furthest from `last`, sets the parity that makes
    `colour` the mover."""
    for shift in (0, 1):
        cells = ref_empty()
        for r, c in discs:
            for below in range(r):
                if (below, c) not in discs:
                    cells[below][c] = filler(below, c, shift)
        for r, c in discs:
            if (r, c) != last:
                cells[r][c] = colour
        assert ref_height(cells, last[1]) == last[0]
        if ref_count(cells) % 2 != colour:
            far = max((c for c in range(COLS) if all(c != col for _, col in discs)), key=lambda c: abs(c - last[1]))
            cells[ref_height(cells, far)][far] = 1 - colour
        assert ref_count(cells) % 2 == colour
        if not ref_finished(cells) and (ref_step(cells, last[1])[1] == 1.0) == wins:
            return cells
    raise AssertionError("no filler leaves this position without a line")


# four in a row on each direction, touching every edge of the board between them: (direction, cells, the last one played)
WINS = [
    ("vertical", [(0, 0), (1, 0), (2, 0), (3, 0)], (3, 0)),           # bottom and left edges
    ("vertical", [(2, 6), (3, 6), (4, 6), (5, 6)], (5, 6)),           # top and right edges
    ("horizontal", [(0, 0), (0, 1), (0, 2), (0, 3)], (0, 0)),         # bottom row from the left edge
    ("horizontal", [(5, 3), (5, 4), (5, 5), (5, 6)], (5, 6)),         # top row to the right edge
    ("horizontal", [(0, 3), (0, 4), (0, 5), (0, 6)], (0, 4)),         # the move closes a gap
    ("rising", [(0, 0), (1, 1), (2, 2), (3, 3)], (3, 3)),             # from the bottom-left corner
    ("rising", [(2, 3), (3, 4), (4, 5), (5, 6)], (2, 3)),             # into the top-right corner
    ("falling", [(3, 0), (2, 1), (1, 2), (0, 3)], (3, 0)),            # left edge down to the bottom row
    ("falling", [(5, 3), (4, 4), (3, 5), (2, 6)], (5, 3)),            # top row down to the right edge
]


@pytest.mark.parametrize("colour", [0, 1])
@pytest.mark.parametrize("case", range(len(WINS)))
def test_wins_on_every_direction_and_edge(case, colour):
    direction, discs, last = WINS[case]
    cells = craft(discs, last, colour, True)
    new, reward, term, illegal = everywhere(cells, last[1])
    assert (reward, term, illegal) == (1.0, True, False) and new[last[0]][last[1]] == colour
    assert (direction, sorted(discs)) in [(n, sorted(line)) for n, line in ref_lines_of(new, colour)]
    # a move on the board that now has a line: illegal in every column, out-of-range actions too, and the board says terminated
    for action in (0, 3, last[1], 6, -1, 7):
        assert everywhere(new, action) == (new, 0.0, True, True)


# What a layout WITHOUT the sentinel bit (6 bits per column) would take for four in a row: its bit index runs from the top of
# column c straight into the bottom of column c + 1.  (r, c) cells of one colour, and the last one played; none of them is a line.
NEAR_MISSES = [
    [(3, 0), (4, 0), (5, 0), (0, 1)],         # "vertical": three at the top of column 0, then the bottom of column 1
    [(3, 5), (4, 5), (5, 5), (0, 6)],         # the same at the right edge
    [(4, 0), (5, 1), (0, 3), (1, 4)],         # "rising": leaves through the top of column 1, re-enters at the bottom of column 3
    [(4, 2), (5, 3), (0, 5), (1, 6)],
    [(1, 0), (0, 1), (5, 1), (4, 2)],         # "falling": leaves through the bottom of column 1, re-enters at its top
    [(1, 4), (0, 5), (5, 5), (4, 6)],
    [(2, 0), (1, 1), (0, 2), (5, 2)],         # ... after three cells
]


@pytest.mark.parametrize("colour", [0, 1])
@pytest.mark.parametrize("case", range(len(NEAR_MISSES)))
def test_lines_do_not_wrap_between_columns(case, colour):
    discs = NEAR_MISSES[case]
    for last in discs:
        if any(r > last[0] and c == last[1] for r, c in discs):
            continue                                                  # (a cell under another of the set cannot be played last)
        cells = craft(discs, last, colour, False)
        new, reward, term, illegal = everywhere(cells, last[1])
        assert (reward, term, illegal) == (0.0, False, False)
        assert all(new[r][c] == colour for r, c in discs) and not ref_finished(new)


def test_full_column_and_actions_out_of_range():
    cells = ref_empty()
    for r in range(ROWS):
        cells[r][2] = filler(r, 2)
    assert ref_count(cells) % 2 == 0 and not ref_finished(cells)
    assert everywhere(cells, 2) == (cells, 0.0, False, True)
    for action in (-1, 7, 1 << 20, -(1 << 20)):
        assert everywhere(cells, action) == (cells, 0.0, False, True)
        assert everywhere(ref_empty(), action) == (ref_empty(), 0.0, False, True)
    new, reward, term, illegal = everywhere(cells, 3)
    assert (reward, term, illegal) == (0.0, False, False) and new[0][3] == 0
    # the first move of a game: colour 0, bottom row
    new, reward, term, illegal = everywhere(ref_empty(), 6)
    assert new[0][6] == 0 and ref_count(new) == 1 and float(ref_obs(new)[42]) == -1.0 and float(ref_obs(new)[6]) == 1.0


def draw_position():
    """A full board without a line, less one top disc of the colour that is to move with 41 discs on the board (colour 1)."""
    cells = [[filler(r, c) for c in range(COLS)] for r in range(ROWS)]
    assert not ref_lines_of(cells, 0) and not ref_lines_of(cells, 1) and ref_finished(cells)
    assert cells[5][1] == 41 % 2
    cells[5][1] = None
    return cells, 1


def test_the_draw():
    cells, column = draw_position()
    assert not ref_finished(cells)
    new, reward, term, illegal = everywhere(cells, column)
    assert (reward, term, illegal) == (0.0, True, False) and ref_count(new) == 42 and new[5][1] == 1
    assert not ref_lines_of(new, 0) and not ref_lines_of(new, 1)
    for action in range(-1, 8):                                       # the full board: finished, every action illegal
        assert everywhere(new, action) == (new, 0.0, True, True)
    for action in (0, 2, 3, 4, 5, 6):                                 # before the last move: six full columns
        assert everywhere(cells, action) == (cells, 0.0, False, True)


# ---- random play ----------------------------------------------------------------------------------------------------------
GAMES, STEPS, AFTER_END = 40, 50, 3


def random_actions(seed):
    """[STEPS][GAMES] actions skewed towards three columns (so that columns fill up), a few of them -1 and 7."""
    g = np.random.RandomState(seed)
    a = g.choice(7, size=(STEPS, GAMES), p=[0.04, 0.08, 0.30, 0.26, 0.24, 0.04, 0.04])
    a[g.rand(STEPS, GAMES) < 0.03] = -1
    a[g.rand(STEPS, GAMES) < 0.03] = 7
    return a


def test_random_play_agrees_everywhere():
    """40 games from a fixed RandomState, each played until AFTER_END moves past its end: the C core, HostConnect4, Connect4Batch
    and the restatement agree on board, observation, reward, terminated and illegal at every move of every game."""
    lib, he = _pkg("_lib").load(), _pkg("host_envs")
    actions = random_actions(4)
    # what the games must contain, counted on the restatement alone before anything is compared
    cover = dict(wins=[0, 0], full_column=0, out_of_range=0, after_end=0, draws=0)
    trace = []
    for e in range(GAMES):
        cells, past, steps = ref_empty(), 0, []
        for t in range(STEPS):
            a = int(actions[t, e])
            was_over = ref_finished(cells)
            mover = ref_count(cells) % 2
            new, reward, term, illegal = ref_step(cells, a)
            steps.append((a, new, reward, term, illegal))
            cover["wins"][mover] += reward == 1.0
            cover["out_of_range"] += a not in range(COLS)
            cover["full_column"] += illegal and not was_over and a in range(COLS) and ref_height(cells, a) == ROWS
            cover["after_end"] += illegal and was_over
            cells = new
            past += was_over
            if past == AFTER_END:
                break
        trace.append(steps)
    assert cover["wins"][0] >= 1 and cover["wins"][1] >= 1 and cover["full_column"] >= 1, cover
    assert cover["out_of_range"] >= 1 and cover["after_end"] >= 1, cover          # games that end with illegal moves still to come
    # the comparison
    cst = [[0, 0] for _ in range(GAMES)]
    single = [he.HostConnect4() for _ in range(GAMES)]
    batch_envs = [he.HostConnect4() for _ in range(GAMES)]
    batch = he.HostConnect4.make_batch(batch_envs)
    for e in range(GAMES):
        obs, _ = single[e].reset(seed=e)
        bobs = batch.reset_one(e, 1000 + e)                         # (the seed is ignored)
        assert np.array_equal(obs, ref_obs(ref_empty())) and np.array_equal(bobs, obs) and obs.dtype == np.float32
    for t in range(max(len(s) for s in trace)):
        go = np.array([t < len(trace[e]) for e in range(GAMES)])
        obs_b, r_b, term_b, ill_b = batch.step_batch(actions[t], go.copy())
        for e in np.nonzero(go)[0].tolist():
            a, new, reward, term, illegal = trace[e][t]
            w = words(new)
            got = c_step(lib, cst[e], a)
            assert got == (w, reward, term, illegal), (t, e)
            cst[e] = got[0]
            if illegal:
                with pytest.raises(ValueError):
                    single[e].step(a)
            else:
                o, rs, ts, trunc, _ = single[e].step(a)
                assert (rs, ts, trunc) == (reward, term, False), (t, e)
                assert np.array_equal(o, ref_obs(new)), (t, e)
            assert [int(x) for x in single[e].discs] == w, (t, e)
            assert (float(r_b[e]), bool(term_b[e]), bool(ill_b[e])) == (reward, term, illegal), (t, e)
            assert np.array_equal(obs_b[e], ref_obs(new)), (t, e)
            assert batch.discs[e].tolist() == w and [int(x) for x in batch_envs[e].discs] == w, (t, e)
        assert not ill_b[~go].any()
