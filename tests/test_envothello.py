"""The Othello rules on the host -- smz_othello_host_step, smz_othello_host_moves (the rule core of csrc/smz_othello.hpp that
the device env compiles too), host_envs.HostOthello and host_envs.OthelloBatch -- against the plain-Python restatement of
tests/othello_ref.py (cells and rays, no bitboards), bit for bit: position, mover, legal mask, reward, terminated and illegal
at every step of 2 000 random games, and on crafted positions."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import othello_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name):
    spec = importlib.util.spec_from_file_location("smz_only_" + name, os.path.join(ROOT, "stochastic-muzero_amd", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def he():
    return _module("host_envs")


@pytest.fixture(scope="module")
def core():
    lib_mod = _module("_lib")
    so = os.path.join(ROOT, "stochastic-muzero_amd", "libsmz.so")
    if not os.path.exists(so):
        pytest.fail("libsmz.so is not built (python __graft_entry__.py build)")
    lib = C.CDLL(so)
    for name in ("smz_othello_host_step", "smz_othello_host_moves"):
        res, args = lib_mod.SIGNATURES[name]
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def c_step(core, d, mover, action):
    """-> (discs, mover, reward, terminated, illegal) of smz_othello_host_step on a copy."""
    w, m = (C.c_uint64 * 2)(*d), C.c_int(mover)
    r, t, i = C.c_float(7.0), C.c_int(-1), C.c_int(-1)
    assert core.smz_othello_host_step(w, C.byref(m), int(action), C.byref(r), C.byref(t), C.byref(i)) == 0
    return [int(w[0]), int(w[1])], m.value, r.value, t.value, i.value


def c_moves(core, d, colour):
    w, out = (C.c_uint64 * 2)(*d), C.c_uint64(1)
    assert core.smz_othello_host_moves(w, colour, C.byref(out)) == 0
    return int(out.value)


def host_at(he, cells, mover):
    env = he.HostOthello()
    env.discs[:] = R.words(cells)
    env.mover[0] = mover
    return env


def check_step(he, core, cells, mover, action, both=None):
    """One action on one position through the restatement, the C core, HostOthello and a one-env OthelloBatch; -> the
    restatement's (cells, mover, reward, terminated, illegal)."""
    d = R.words(cells)
    want = R.step(cells, mover, action, both)
    new, mover2, reward, term, illegal = want
    assert c_step(core, d, mover, action) == (R.words(new), mover2, reward, int(term), int(illegal)), (d, mover, action)
    for colour in (0, 1):
        assert c_moves(core, d, colour) == R.mask(cells, colour), (d, colour)
    env = host_at(he, cells, mover)
    assert env.legal_moves() == R.mask(cells, mover) and env.legal_moves(1 - mover) == R.mask(cells, 1 - mover)
    try:
        o, r, t = env.step(action)[:3]
        assert not illegal and (r, t) == (reward, term) and np.array_equal(o, R.obs(new, mover2)), (d, mover, action)
    except ValueError:
        assert illegal, (d, mover, action)
    assert env.discs.tolist() == R.words(new) and int(env.mover[0]) == mover2
    batch = he.OthelloBatch([host_at(he, cells, mover)])
    o, r, t, i = batch.step_batch(np.array([action]), np.array([True]))
    assert batch.discs[0].tolist() == R.words(new) and int(batch.mover[0]) == mover2, (d, mover, action)
    assert (float(r[0]), bool(t[0]), bool(i[0])) == (reward, term, illegal) and np.array_equal(o[0], R.obs(new, mover2))
    return want


def test_two_thousand_random_games_agree_bit_for_bit(he, core):
    """The mover picks uniformly among the restatement's legal actions; one random action in -1 .. 66 is interleaved per game.
    All games advance in lockstep, so OthelloBatch steps them as ONE slice (finished games with go = False)."""
    n = 2000
    g = np.random.RandomState(2022)
    cells, mover = [R.start() for _ in range(n)], [0] * n
    both = [(R.placements(c, 0), R.placements(c, 1)) for c in cells]
    live = [True] * n
    odd_at = g.randint(0, 60, n)                              # the round at which a game gets its random action
    singles = [he.HostOthello() for _ in range(n)]
    batch = he.OthelloBatch([he.HostOthello() for _ in range(n)])
    assert isinstance(he.HostOthello.make_batch([he.HostOthello()]), he.OthelloBatch)
    cover = dict(passes=0, early=0, wins=[0, 0], draws=0, illegal=0, steps=0)
    rounds = 0
    while any(live):
        actions, go = np.zeros(n, np.int64), np.array(live)
        for e in range(n):
            if live[e]:
                legal = R.legal_actions(cells[e], mover[e], both[e])
                actions[e] = g.randint(-1, 67) if rounds == odd_at[e] else legal[g.randint(len(legal))]
        before = [(batch.discs[e].tolist(), int(batch.mover[e])) for e in range(n)]
        o_b, r_b, t_b, i_b = batch.step_batch(actions, go)
        for e in range(n):
            if not live[e]:
                assert (batch.discs[e].tolist(), int(batch.mover[e])) == before[e] and not i_b[e]
                continue
            a, d = int(actions[e]), R.words(cells[e])
            for colour in (0, 1):
                m = sum(1 << sq for sq in both[e][colour])
                assert c_moves(core, d, colour) == m, (e, rounds)
                assert colour != mover[e] or singles[e].legal_moves() == m, (e, rounds)
            new, mover2, reward, term, illegal = R.step(cells[e], mover[e], a, both[e])
            assert c_step(core, d, mover[e], a) == (R.words(new), mover2, reward, int(term), int(illegal)), (e, rounds, a)
            want_obs = R.obs(new, mover2)
            try:
                o, r, t = singles[e].step(a)[:3]
                assert not illegal and (r, t) == (reward, term) and np.array_equal(o, want_obs), (e, rounds, a)
            except ValueError:
                assert illegal, (e, rounds, a)
            assert singles[e].discs.tolist() == R.words(new) and int(singles[e].mover[0]) == mover2, (e, rounds, a)
            assert batch.discs[e].tolist() == R.words(new) and int(batch.mover[e]) == mover2, (e, rounds, a)
            assert (float(r_b[e]), bool(t_b[e]), bool(i_b[e])) == (reward, term, illegal), (e, rounds, a)
            assert np.array_equal(o_b[e], want_obs), (e, rounds, a)
            cover["steps"] += 1
            cover["illegal"] += illegal
            if not illegal:
                cover["passes"] += a == R.PASS
                if new is not cells[e]:
                    both[e] = (R.placements(new, 0), R.placements(new, 1))
                if term:
                    live[e] = False
                    cover["early"] += R.count(new) < 64
                    cover["draws"] += reward == 0.0
                    if reward != 0.0:
                        cover["wins"][mover[e] if reward > 0 else 1 - mover[e]] += 1
                cells[e], mover[e] = new, mover2
        rounds += 1
    print(cover, rounds)
    assert cover["passes"] >= 1 and cover["early"] >= 1 and cover["wins"][0] >= 1 and cover["wins"][1] >= 1, cover
    assert cover["draws"] >= 1 and cover["illegal"] >= 1, cover


def test_the_start_position_and_reset(he, core):
    env = he.HostOthello()
    o, info = env.reset(seed=5)
    assert env.discs.tolist() == R.words(R.start()) and int(env.mover[0]) == 0 and info == {}
    assert np.array_equal(o, R.obs(R.start(), 0)) and o.dtype == np.float32 and o.shape == (65,)
    assert sorted(R.placements(R.start(), 0)) == [19, 26, 37, 44] and c_moves(core, R.words(R.start()), 0) == R.mask(R.start(), 0)
    env.step(19)
    env.reset()
    assert env.discs.tolist() == R.words(R.start()) and int(env.mover[0]) == 0
    assert np.array_equal(he.othello_observations(np.array([R.words(R.start())], np.uint64), [1])[0], R.obs(R.start(), 1))


def test_a_placement_that_flips_in_all_eight_directions(he, core):
    cells, mover, action = R.all_directions()
    new, mover2, reward, term, illegal = check_step(he, core, cells, mover, action)
    assert not illegal and mover2 == 1 and R.count(new, 0) - R.count(cells, 0) == 19 and R.count(new, 1) == 0 and term
    assert reward == 1.0


def test_a_wipe_out_ends_the_game_before_the_board_is_full(he, core):
    cells, mover, action = R.wipe_out()
    new, _, reward, term, illegal = check_step(he, core, cells, mover, action)
    assert (reward, term, illegal) == (1.0, True, False) and R.count(new) == 3 and R.count(new, 1) == 0


def test_runs_reach_the_a_and_h_files_without_wrapping(he, core):
    for cells, mover, action, legal in R.edge_runs():
        assert not R.finished(cells)
        new, _, _, _, illegal = check_step(he, core, cells, mover, action)
        assert illegal == (not legal), action
        if legal:
            assert R.count(new, mover) - R.count(cells, mover) == 7, action          # the disc and six flips
        for a in range(-1, 67):                               # and every other action on these positions
            check_step(he, core, cells, mover, a)
            check_step(he, core, cells, 1 - mover, a)


def test_a_pass_is_refused_while_a_placement_exists_and_taken_when_none_does(he, core):
    cells, mover, action = R.refused_pass()
    assert check_step(he, core, cells, mover, action)[4] is True
    cells, mover, action = R.legal_pass()
    new, mover2, reward, term, illegal = check_step(he, core, cells, mover, action)
    assert new is cells and (mover2, reward, term, illegal) == (0, 0.0, False, False)
    for a in range(0, 64):                                    # the side that must pass can place nothing
        assert check_step(he, core, cells, mover, a)[4] is True
    new, _, reward, term, illegal = check_step(he, core, cells, 0, 2)               # and the other side then takes the last disc
    assert (reward, term, illegal) == (1.0, True, False) and R.count(new, 1) == 0


def test_every_action_is_refused_on_a_finished_position(he, core):
    cells, mover = R.finished_position()
    full = R.from_rows(["xxxxoooo"] * 8)
    for position in (cells, full):
        for m in (0, 1):
            for a in list(range(-2, 68)) + [1 << 30, -(1 << 31)]:
                assert check_step(he, core, position, m, a)[2:] == (0.0, True, True), (m, a)


def test_host_step_refuses_null_arguments(core):
    m = C.c_int(0)
    w = (C.c_uint64 * 2)(*R.words(R.start()))
    assert core.smz_othello_host_step(None, C.byref(m), 19, None, None, None) != 0
    assert core.smz_othello_host_step(w, None, 19, None, None, None) != 0
    assert core.smz_othello_host_moves(w, 2, C.byref(C.c_uint64())) != 0 and core.smz_othello_host_moves(w, 0, None) != 0
    assert core.smz_othello_host_step(w, C.byref(m), 19, None, None, None) == 0 and m.value == 1      # outputs may be NULL
    assert [int(w[0]), int(w[1])] == R.words(R.step(R.start(), 0, 19)[0])
