"""The step kernel the device board games share (csrc/smz_env_frame.hpp: k_board_step_env over Game2048 and GameConnect4) at its
workgroup edges and with its nullable arguments: a step with and without the trajectory record leaves the same env behind,
both play the host twin's games, and a call without the observation, reward and flag outputs moves the same state and writes
the same record."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, LIMIT, SEED = 12, 5, 7
GAMES = {"2048": dict(dev="Board2048Vec", host="Host2048", obs=16, A=4, state=("board", "spawns"), step="smz_2048_step_ctl"),
         "connect4": dict(dev="Connect4Vec", host="HostConnect4", obs=43, A=7, state=("discs",), step="smz_connect4_step_ctl")}
TENSORS = ("obs", "reward", "terminated", "step_count", "episode", "active")


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _inputs(game, B):
    """Seeded actions from -1 .. A (both ends are out of range; the last env gets one of each for certain) and search outputs."""
    g = np.random.RandomState(1000 * B + game["A"])
    actions = g.randint(-1, game["A"] + 1, size=(T, B)).astype(np.int32)
    actions[1, -1], actions[2, -1] = -1, game["A"]
    out = (torch.from_numpy(g.rand(B, game["A"])).to(DEV), torch.from_numpy(g.rand(B, game["A"])).to(DEV),
           torch.from_numpy(g.randn(B).astype(np.float32)).to(DEV))
    return actions, out


def _snapshot(env, game):
    return {k: None if getattr(env, k) is None else getattr(env, k).cpu().numpy().copy() for k in TENSORS + game["state"]}


def _device_run(game, B, on_end, actions, out, record):
    """-> (the env, its tensors after every step, the chunk or None)"""
    env = getattr(_pkg("envs"), game["dev"])(B, DEV, seed=SEED, on_end=on_end, limit=LIMIT)
    env.reset()
    chunk = torch.full((T, B, game["obs"] + 3 * game["A"] + 3), -5.0, dtype=torch.float64, device=DEV) if record else None
    steps = []
    for t in range(T):
        act = torch.from_numpy(actions[t]).to(DEV)
        if record:
            env.step_and_record(act, chunk, t, *out)
        else:
            env.step(act)
        torch.cuda.synchronize()
        steps.append(_snapshot(env, game))
    return env, steps, None if chunk is None else chunk.cpu().numpy()


def _host_run(game, B, on_end, actions, out):
    envs, sp = _pkg("envs"), _pkg("selfplay")
    env = envs.HostVecEnv([getattr(envs, game["host"])] * B, game["obs"], game["A"], DEV, env_seed=SEED, limit=LIMIT, on_end=on_end,
                          workers=0)
    try:
        env.reset()
        chunk = sp.TrajectoryChunk(T, B, game["obs"], game["A"], env.device)
        for t in range(T):
            act = torch.from_numpy(actions[t]).to(DEV)
            env.step_begin(act)
            sp._record_phase(env, chunk, t, (act,) + tuple(out))
        torch.cuda.synchronize()
        return chunk.data.cpu().numpy()
    finally:
        env.close()


@pytest.mark.parametrize("on_end", ["mask", "reset"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("name", sorted(GAMES))
def test_step_and_step_with_record_play_the_host_twins_games(name, B, on_end):
    game = GAMES[name]
    OBS = game["obs"]
    actions, out = _inputs(game, B)
    assert (actions == -1).any() and (actions == game["A"]).any()
    _, plain, _ = _device_run(game, B, on_end, actions, out, record=False)
    _, recorded, dev = _device_run(game, B, on_end, actions, out, record=True)
    for t in range(T):
        for k in TENSORS + game["state"]:
            if plain[t][k] is None:
                assert recorded[t][k] is None and k == "active" and on_end == "reset"
            else:
                assert np.array_equal(plain[t][k], recorded[t][k]), (t, k)
    host = _host_run(game, B, on_end, actions, out)
    flags, rewards = host[..., OBS + 1], host[..., OBS]
    for run in (plain, recorded):
        assert np.array_equal(np.stack([s["terminated"] for s in run]), flags)
        assert np.array_equal(np.stack([s["reward"] for s in run]), rewards)
    # the record, as test_host_twin_plays_the_same_games compares it: every row of a game is equal; a switched-off env takes no
    # step, and its rows are compared on flag and reward only
    stepped = flags != 3
    assert np.array_equal(dev[..., OBS + 1], flags) and np.array_equal(dev[stepped], host[stepped])
    assert np.array_equal(dev[..., OBS][~stepped], rewards[~stepped])
    assert (rewards < 0).any() and (flags == 2).any()         # illegal moves, the limit
    assert (flags[LIMIT:] == 3).all() and stepped[:LIMIT].all() if on_end == "mask" else stepped.all()


@pytest.mark.parametrize("name", sorted(GAMES))
def test_a_step_without_its_outputs_moves_the_same_state_and_writes_the_same_record(name):
    """obs_out_dev, reward_out_dev and flag_out_dev all null."""
    game, B, lib_mod = GAMES[name], 65, _pkg("_lib")
    actions, out = _inputs(game, B)
    want_env, _, want = _device_run(game, B, "reset", actions, out, record=True)
    env = getattr(_pkg("envs"), game["dev"])(B, DEV, seed=SEED, on_end="reset", limit=LIMIT)
    env.reset()
    torch.cuda.synchronize()
    before = _snapshot(env, game)
    chunk = torch.full((T, B, want.shape[2]), -5.0, dtype=torch.float64, device=DEV)
    P = lambda x: C.c_void_p(x.data_ptr())
    step = getattr(lib_mod.load(), game["step"])
    for t in range(T):
        act = torch.from_numpy(actions[t]).to(DEV)
        lib_mod.check(step(*(P(getattr(env, k)) for k in game["state"]), P(act), None, None, None, C.byref(env._ctl_struct()),
                           P(chunk), T, t, P(out[0]), P(out[1]), P(out[2]), B, None))
        torch.cuda.synchronize()
    after = _snapshot(env, game)
    for k in ("obs", "reward", "terminated"):
        assert np.array_equal(after[k], before[k]), k         # untouched
    for k in ("step_count", "episode") + game["state"]:
        assert np.array_equal(after[k], getattr(want_env, k).cpu().numpy()), k
    assert np.array_equal(chunk.cpu().numpy(), want)
