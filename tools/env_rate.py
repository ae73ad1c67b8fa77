"""What a device-resident board game costs and what it buys: envs.Board2048Vec against host_envs.Host2048 (--game 2048), or
envs.Connect4Vec against host_envs.HostConnect4 under the two-player search (--game connect4), or envs.OthelloVec against
host_envs.HostOthello under the two-player search on a large-action handle (--game othello), the host envs behind HostVecEnv.

Everything at `--envs` environments (4096), one GPU:
  step      the env step launch alone (smz_2048_step_ctl / smz_connect4_step_ctl / smz_othello_step_ctl with its trajectory
            record, on_end "reset"):
            `--steps` launches back to back on one stream between two device events, uploaded random actions; three blocks, the
            median is reported.  That figure is the rate at which this process can issue the launch (the host's enqueue
            included), not a kernel time; the kernel time comes from the profiler, in a run of its own:
                rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/env_rate.py --game G --only step
  selfplay  simulations/s of self-play (selfplay.play_games: search + action + env step + record per env step) with a fresh
            mlp_model that fits LDS (the game's obs and A, S 31, H 64, L 0: for 2048 the checkpoint-421 widths), `--sims`
            simulations (50), on_end "reset": on the device env, and on HostVecEnv([host env] * envs, workers=W) for every W of
            --workers (2048: 0,8,14; connect4 and othello: 0,8).  One warm-up chunk, then five blocks of `--chunks` chunks of `--chunk` env
            steps, each block between synchronisations (16 x 32 steps: a fifth of a second or more); the median block is
            reported, min and max printed.
            connect4 plays with number_of_player = 2 and limit 42, once for each search of --searches (stepwise: the step-wise
            multi-player search; single: players_single_launch=True).  With workers the move counters live in the worker
            processes, and the two-player search takes its root player from them: the tool keeps a device copy for those cells
            (one in-place tensor update per env step, from the uploaded flags: under on_end "reset" the counter restarts
            whenever the flag is non-zero).
            othello plays with number_of_player = 2 and limit 120 on a large-action handle (65 actions), step-wise only: the
            large-action single launch (smz_search_mlp_large) is one player only, so --searches is "stepwise" for this game.
Prints one JSON line per measurement and, with --out, appends the same lines to a file.

    python tools/env_rate.py --game 2048|connect4|othello [--envs 4096] [--sims 50] [--workers 0,8] [--searches stepwise,single]
                             [--only step|selfplay] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# device class, host class, obs, A, limit of the self-play games, players, default --workers, default --searches
GAMES = {"2048": dict(dev="Board2048Vec", host="Host2048", obs=16, A=4, limit=0, players=1, workers="0,8,14"),
         "connect4": dict(dev="Connect4Vec", host="HostConnect4", obs=43, A=7, limit=42, players=2, workers="0,8",
                          searches="stepwise,single"),
         "othello": dict(dev="OthelloVec", host="HostOthello", obs=65, A=65, limit=120, players=2, workers="0,8",
                         searches="stepwise")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=sorted(GAMES), required=True)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30000)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--only", choices=("step", "selfplay"), default=None)
    ap.add_argument("--workers", default=None)
    ap.add_argument("--searches", default=None, help="two-player games: stepwise,single (connect4); stepwise (othello: the "
                    "large-action single launch is one player only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a rate is measured on the GPU or not at all"
    import stochastic_muzero_amd  # noqa: F401
    envs_mod, sp, mcts_mod, model_mod = (import_module("stochastic-muzero_amd." + m) for m in ("envs", "selfplay", "mcts", "model"))
    game, dev, B = GAMES[a.game], "cuda:0", a.envs
    if a.workers is None:
        a.workers = game["workers"]
    if a.searches is None:
        a.searches = game.get("searches", "")
    assert a.game != "othello" or a.searches == "stepwise", "a two-player search on a large-action handle is step-wise"
    name = torch.cuda.get_device_name(0)

    def emit(**rec):
        line = json.dumps(dict(rec, envs=B, device=name))
        print(line, flush=True)
        if a.out:                                             # line by line: a cell that fails leaves the earlier ones on file
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.only != "selfplay":
        step_launch(a, game, envs_mod, dev, B, emit)
    if a.only != "step":
        self_play(a, game, envs_mod, sp, mcts_mod, model_mod, dev, B, emit)


def step_launch(a, game, envs_mod, dev, B, emit):
    A, F = game["A"], game["obs"] + 3 * game["A"] + 3
    env = getattr(envs_mod, game["dev"])(B, dev, seed=0, on_end="reset")
    env.reset()
    g = np.random.RandomState(0)
    pool = [torch.from_numpy(g.randint(0, A, B).astype(np.int32)).to(dev) for _ in range(64)]
    T = 64
    chunk = torch.zeros(T, B, F, dtype=torch.float64, device=dev)
    policy, visits = torch.rand(B, A, dtype=torch.float64, device=dev), torch.rand(B, A, dtype=torch.float64, device=dev)
    root_value = torch.rand(B, device=dev)
    for t in range(200):
        env.step_and_record(pool[t % 64], chunk, t % T, policy, visits, root_value)
    torch.cuda.synchronize()
    blocks = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(a.steps):
            env.step_and_record(pool[t % 64], chunk, t % T, policy, visits, root_value)
        e1.record()
        torch.cuda.synchronize()
        blocks.append(1e3 * e0.elapsed_time(e1) / a.steps)
    emit(what="step", us_per_step_launch=round(float(np.median(blocks)), 3), blocks_us=[round(b, 3) for b in blocks],
         launches_per_block=a.steps, games_finished=int(env.episode.sum()))


class DeviceMoveCounter:
    """A HostVecEnv whose move counters live in worker processes, with a device copy of them for the two-player search's root
    player (module docstring).  Everything else is the wrapped env's."""

    def __init__(self, env):
        assert env.on_end == "reset"
        self._env = env
        self.step_count = torch.zeros(env.B, dtype=torch.int32, device=env.device)

    def __getattr__(self, name):
        return getattr(self._env, name)

    def reset(self):
        self.step_count.zero_()
        return self._env.reset()

    def step_end(self):
        out = self._env.step_end()
        self.step_count.add_(1).masked_fill_(out[2] != 0, 0)
        return out


def self_play(a, game, envs_mod, sp, mcts_mod, model_mod, dev, B, emit):
    obs, A, limit, two = game["obs"], game["A"], game["limit"], game["players"] == 2
    with torch.random.fork_rng():
        torch.manual_seed(0)
        model = model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=obs, action_space_dimensions=A,
                                 state_space_dimensions=31, hidden_layer_dimensions=64, number_of_hidden_layer=0, random_tag=0)
    heads = model.heads(dev)

    def selfplay(env, label, search, **extra):
        """search: None (the single-player search) or, with two players, "stepwise" / "single"."""
        players, cell = {}, {}
        if search is not None:
            players = dict(number_of_player=2, players_single_launch=search == "single")
            cell, extra = dict(search=search), dict(extra, heads=type(heads).__name__)
        env.reset()
        m = mcts_mod.BatchedMCTS(B, num_simulations=a.sims, discount=0.997, root_exploration_fraction=0.1, **players)
        m.seed(np.arange(B, dtype=np.uint64))
        sp.play_games(env, heads, m, 1.0, a.chunk)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(a.chunks):
                sp.play_games(env, heads, m, 1.0, a.chunk)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / (a.chunk * a.chunks))
        ms = 1e3 * float(np.median(ts))
        emit(what="selfplay", env=label, **cell, sims=a.sims, ms_per_env_step=round(ms, 3),
             simulations_per_s=round(B * a.sims / (ms * 1e-3)), min_ms=round(1e3 * min(ts), 3), max_ms=round(1e3 * max(ts), 3),
             env_steps_per_block=a.chunk * a.chunks, single_launch=m._single is True,
             kernel=m.engine.last_kernel() if m._single is True else "", **extra)
        m.engine.close()

    host_class = getattr(envs_mod, game["host"])
    for search in ([s for s in a.searches.split(",") if s] if two else [None]):
        assert search in (None, "stepwise", "single"), search
        selfplay(getattr(envs_mod, game["dev"])(B, dev, seed=0, on_end="reset", limit=limit), game["dev"], search)
        for w in [int(x) for x in a.workers.split(",") if x != ""]:
            henv = envs_mod.HostVecEnv([host_class] * B, obs, A, dev, env_seed=0, on_end="reset", limit=limit, workers=w)
            try:
                selfplay(DeviceMoveCounter(henv) if two and w else henv, "HostVecEnv(%s)" % game["host"], search, workers=w)
            finally:
                henv.close()


if __name__ == "__main__":
    main()
