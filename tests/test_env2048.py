"""The rules of the 2048 environment on the CPU: the C rule core compiled for the host (smz_2048_host_step / _host_reset),
host_envs.Host2048 and host_envs.Board2048Batch against a plain-Python restatement written here from the rules as
include/smz.h states them (a per-line loop; it imports neither Board2048Batch nor the C core)."""
import ctypes as C
import math
from importlib import import_module

import numpy as np
import pytest


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


# ---- the restatement ------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def ref_mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ref_unit(seed, env, epoch, comp):
    z = ref_mix64((seed ^ (env * 0xD1342543DE82EF95)) & M64)
    z = ref_mix64((z + epoch) & M64)
    z = ref_mix64((z + comp) & M64)
    return (z >> 11) / 9007199254740992.0


def ref_line(line):
    """One line, index 0 = the edge the tiles move towards -> (new line, values of the tiles the merges created)."""
    tiles = [v for v in line if v]
    out, gain, i = [], 0, 0
    while i < len(tiles):
        if i + 1 < len(tiles) and tiles[i] == tiles[i + 1]:
            out.append(tiles[i] + 1)
            gain += 2 ** (tiles[i] + 1)
            i += 2
        else:
            out.append(tiles[i])
            i += 1
    return out + [0] * (4 - len(out)), gain


def ref_cell(action, line, j):
    """Board index of position j (0 = at the edge) of line `line` for 0 up, 1 right, 2 down, 3 left."""
    return (4 * j + line, 4 * line + 3 - j, 4 * (3 - j) + line, 4 * line + j)[action]


def ref_move(board, action):
    new, gain = list(board), 0
    for line in range(4):
        cells = [ref_cell(action, line, j) for j in range(4)]
        out, g = ref_line([board[c] for c in cells])
        gain += g
        for c, v in zip(cells, out):
            new[c] = v
    return new, gain


def ref_dead(board):
    return all(ref_move(board, a)[0] == list(board) for a in range(4))


def ref_spawn(board, game_seed, n):
    empty = [i for i in range(16) if board[i] == 0]
    u0, u1 = ref_unit(game_seed, 0, n, 0), ref_unit(game_seed, 0, n, 1)
    e = 2 if u1 < 0.1 else 1
    board[empty[int(math.floor(u0 * len(empty)))]] = e
    return e


def ref_reset(game_seed):
    board = [0] * 16
    ref_spawn(board, game_seed, 0)
    ref_spawn(board, game_seed, 1)
    return board, 2


def ref_step(board, spawns, action, game_seed):
    """-> (board, spawns, reward, terminated, illegal, exponent spawned or 0)"""
    board = list(board)
    if action not in (0, 1, 2, 3):
        return board, spawns, 0.0, ref_dead(board), True, 0
    new, gain = ref_move(board, action)
    if new == board:
        return board, spawns, 0.0, ref_dead(board), True, 0
    e = ref_spawn(new, game_seed, spawns)
    return new, spawns + 1, float(gain), ref_dead(new), False, e


# ---- the C core -----------------------------------------------------------------------------------------------------------
def c_step(lib, board, spawns, action, game_seed):
    b = (C.c_uint8 * 16)(*board)
    n, r, term, ill = C.c_int32(spawns), C.c_float(-7.0), C.c_int(-7), C.c_int(-7)
    assert lib.smz_2048_host_step(b, C.byref(n), action, game_seed, C.byref(r), C.byref(term), C.byref(ill)) == 0
    return list(b), n.value, r.value, bool(term.value), bool(ill.value)


def c_reset(lib, game_seed):
    b, n = (C.c_uint8 * 16)(*([9] * 16)), C.c_int32(-1)
    assert lib.smz_2048_host_reset(b, C.byref(n), game_seed) == 0
    return list(b), n.value


def oriented(line, action, other=(0, 0, 0, 0)):
    """A board whose line 0 for `action` is `line` (index 0 at the edge the tiles move towards), `other` in the other lines."""
    board = [0] * 16
    for ln in range(4):
        for j in range(4):
            board[ref_cell(action, ln, j)] = (line if ln == 0 else other)[j]
    return board


@pytest.mark.parametrize("action", [0, 1, 2, 3])
def test_crafted_boards_against_the_host_rule_core(action):
    lib = _pkg("_lib").load()
    seed = 12345
    # tiles 2 and 4 are exponents 1 and 2: [2,2,2,2] -> [4,4,0,0], [2,2,4,0] -> [4,4,0,0], [4,2,2,0] -> [4,4,0,0]; 15 + 15 -> 16
    for line, want, reward in (([1, 1, 1, 1], [2, 2, 0, 0], 8.0), ([1, 1, 2, 0], [2, 2, 0, 0], 4.0),
                               ([2, 1, 1, 0], [2, 2, 0, 0], 4.0), ([15, 15, 0, 0], [16, 0, 0, 0], 65536.0)):
        board = oriented(line, action)
        got, n, r, term, ill = c_step(lib, board, 5, action, seed)
        moved = oriented(want, action)
        assert ref_move(board, action) == (moved, int(reward))
        assert not ill and r == reward and n == 6
        spawned = [i for i in range(16) if got[i] != moved[i]]
        assert len(spawned) == 1 and moved[spawned[0]] == 0 and got[spawned[0]] in (1, 2)
        assert (got, n, r, term, ill) == ref_step(board, 5, action, seed)[:5]
    # a board the move does not change: illegal, nothing written
    stuck = oriented([3, 2, 1, 0], action, other=[1, 2, 0, 0])
    assert c_step(lib, stuck, 7, action, seed) == (stuck, 7, 0.0, False, True)
    # a full board without equal neighbours: every move illegal, terminated
    full = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
    assert c_step(lib, full, 9, action, seed) == (full, 9, 0.0, True, True)
    assert ref_dead(full) and ref_step(full, 9, action, seed)[:5] == (full, 9, 0.0, True, True)
    # actions outside 0 .. 3 index nothing: illegal
    live = oriented([1, 1, 0, 0], action)
    for bad in (4, -1):
        assert c_step(lib, live, 3, bad, seed) == (live, 3, 0.0, False, True)


def test_random_play_agrees_everywhere():
    """32 games of up to 400 moves from a fixed RandomState: the C core, Host2048, Board2048Batch and the restatement agree on
    board, spawns, reward, terminated and illegal at every step of every env."""
    lib = _pkg("_lib").load()
    he = _pkg("host_envs")
    assert he.smz_unit(77, 3, 5, 1) == ref_unit(77, 3, 5, 1) and he.smz_mix64(M64) == ref_mix64(M64)
    B, steps, base = 32, 400, 2024
    seeds = [(base + e) & M64 for e in range(B)]
    rng = np.random.RandomState(7)
    actions = rng.randint(0, 4, size=(steps, B))
    actions[rng.rand(steps, B) < 0.02] = 4                 # a few out of range (the C core and the batch; Host2048 raises)
    actions[rng.rand(steps, B) < 0.01] = -1
    ref = [ref_reset(s) for s in seeds]
    cst = [c_reset(lib, s) for s in seeds]
    single = [he.Host2048() for _ in range(B)]
    batch_envs = [he.Host2048() for _ in range(B)]
    batch = he.Host2048.make_batch(batch_envs)
    assert isinstance(batch, he.Board2048Batch)
    for e in range(B):
        obs, _ = single[e].reset(seed=seeds[e])
        bobs = batch.reset_one(e, seeds[e])
        assert ref[e] == cst[e] and list(single[e].board) == ref[e][0] and single[e].spawns == 2
        assert list(batch.board[e]) == ref[e][0] and batch.spawns[e] == 2
        want = np.array(ref[e][0], np.float32) * np.float32(0.0625)
        assert obs.dtype == np.float32 and np.array_equal(obs, want) and np.array_equal(bobs, want)
    alive = np.ones(B, bool)
    fours = illegals = deaths = 0
    for t in range(steps):
        if not alive.any():
            break
        obs_b, r_b, term_b, ill_b = batch.step_batch(actions[t], alive.copy())
        for e in np.nonzero(alive)[0].tolist():
            a = int(actions[t, e])
            board, n, r, term, ill, spawned = ref_step(ref[e][0], ref[e][1], a, seeds[e])
            assert c_step(lib, cst[e][0], cst[e][1], a, seeds[e]) == (board, n, np.float32(r), term, ill), (t, e)
            if ill:
                with pytest.raises(ValueError):
                    single[e].step(a)
                assert bool(ill_b[e])
            else:
                o, rs, ts, trunc, _ = single[e].step(a)
                assert (rs, ts, trunc) == (r, term, False), (t, e)
                assert np.array_equal(o, np.array(board, np.float32) * np.float32(0.0625))
                assert (r_b[e], bool(term_b[e]), bool(ill_b[e])) == (r, term, False), (t, e)
                assert np.array_equal(obs_b[e], o)
            assert list(single[e].board) == board and single[e].spawns == n, (t, e)
            assert list(batch.board[e]) == board and batch.spawns[e] == n, (t, e)
            assert list(batch_envs[e].board) == board               # the env object's board is a view of the batch's row
            ref[e], cst[e] = (board, n), (board, n)
            fours += spawned == 2
            illegals += ill
            if term:
                deaths += 1
                alive[e] = False
    # the run must have met every rule (counted on the restatement's side)
    assert fours >= 1 and illegals >= 1 and deaths >= 1, (fours, illegals, deaths)
