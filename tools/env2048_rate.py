"""What the device-resident 2048 env costs and what it buys (envs.Board2048Vec against host_envs.Host2048 behind HostVecEnv).

Everything at `--envs` environments (4096), one GPU:
  step      the env step launch alone (smz_2048_step_ctl with its trajectory record, on_end "reset"): `--steps` launches back to
            back on one stream between two device events, uploaded random actions; three blocks, the median is reported.  That
            figure is the rate at which this process can issue the launch (the host's enqueue included), not a kernel time;
            the kernel time comes from the profiler, in a run of its own:
                rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/env2048_rate.py --only step
  selfplay  simulations/s of self-play (selfplay.play_games: search + action + env step + record per env step) with a fresh
            mlp_model of the checkpoint-421 widths (obs 16, A 4, S 31, H 64, L 0), `--sims` simulations (50), on_end "reset":
            on Board2048Vec, and on HostVecEnv([Host2048] * envs, workers=W) for every W of --workers.  One warm-up chunk, then
            five blocks of `--chunks` chunks of `--chunk` env steps, each block between synchronisations (16 x 32 steps: a fifth
            of a second or more); the median block is reported, min and max printed.
Prints one JSON line per measurement and, with --out, appends the same lines to a file.

    python tools/env2048_rate.py [--envs 4096] [--sims 50] [--workers 0,8,14] [--only step|selfplay] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30000)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--only", choices=("step", "selfplay"), default=None)
    ap.add_argument("--workers", default="0,8,14")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a rate is measured on the GPU or not at all"
    import stochastic_muzero_amd  # noqa: F401
    envs_mod, sp, mcts_mod, model_mod = (import_module("stochastic-muzero_amd." + m) for m in ("envs", "selfplay", "mcts", "model"))
    dev, B = "cuda:0", a.envs
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(**rec):
        lines.append(json.dumps(dict(rec, envs=B, device=name)))
        print(lines[-1], flush=True)

    def finish():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    if a.only != "selfplay":
        step_launch(a, envs_mod, dev, B, emit)
    if a.only != "step":
        self_play(a, envs_mod, sp, mcts_mod, model_mod, dev, B, emit)
    finish()


def step_launch(a, envs_mod, dev, B, emit):
    env = envs_mod.Board2048Vec(B, dev, seed=0, on_end="reset")
    env.reset()
    g = np.random.RandomState(0)
    pool = [torch.from_numpy(g.randint(0, 4, B).astype(np.int32)).to(dev) for _ in range(64)]
    T = 64
    chunk = torch.zeros(T, B, 31, dtype=torch.float64, device=dev)
    policy, visits = torch.rand(B, 4, dtype=torch.float64, device=dev), torch.rand(B, 4, dtype=torch.float64, device=dev)
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


def self_play(a, envs_mod, sp, mcts_mod, model_mod, dev, B, emit):
    with torch.random.fork_rng():
        torch.manual_seed(0)
        model = model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=16, action_space_dimensions=4,
                                 state_space_dimensions=31, hidden_layer_dimensions=64, number_of_hidden_layer=0, random_tag=0)
    heads = model.heads(dev)

    def selfplay(env, label, **extra):
        env.reset()
        m = mcts_mod.BatchedMCTS(B, num_simulations=a.sims, discount=0.997, root_exploration_fraction=0.1)
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
        emit(what="selfplay", env=label, sims=a.sims, ms_per_env_step=round(ms, 3), simulations_per_s=round(B * a.sims / (ms * 1e-3)),
             min_ms=round(1e3 * min(ts), 3), max_ms=round(1e3 * max(ts), 3), env_steps_per_block=a.chunk * a.chunks,
             single_launch=m._single is True, kernel=m.engine.last_kernel() if m._single is True else "", **extra)
        m.engine.close()

    selfplay(envs_mod.Board2048Vec(B, dev, seed=0, on_end="reset"), "Board2048Vec")
    for w in [int(x) for x in a.workers.split(",") if x != ""]:
        henv = envs_mod.HostVecEnv([envs_mod.Host2048] * B, 16, 4, dev, env_seed=0, on_end="reset", workers=w)
        try:
            selfplay(henv, "HostVecEnv(Host2048)", workers=w)
        finally:
            henv.close()


if __name__ == "__main__":
    main()
