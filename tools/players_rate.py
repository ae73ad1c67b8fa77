"""Search rate of multi-player mlp_model searches (HipMlpHeads): the step-wise graph path against the single launch.

Shapes: the reference's checkpoint-421 net (S 31, H 64, L 0, 2 actions) with number_of_player=2 at 4096 and 1024 trees, and one
fresh 9-action net (obs 12, S 21, H 32, L 0) with number_of_player=3 at 4096 trees; 50 simulations, train=True, root players
arange(B) mod the cycle length.  Per shape, in the same call and with the same heads: the step-wise search replayed as one HIP
graph, and BatchedMCTS(players_single_launch=True) (one smz_search_mlp_players launch per search).  Each: one warm-up search,
then three blocks of `--searches` searches between synchronisations (200: a block times a quarter of a second or more);
the median block is reported, all three are printed.  Prints one JSON line per
measurement and, with --out, appends the same lines to a file.

    python tools/players_rate.py [--sims 50] [--searches 200] [--out FILE]
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
# (name, players, trees)
SHAPES = (("ckpt421", 2, 4096), ("ckpt421", 2, 1024), ("fresh_a9", 3, 4096))


def net(name, model_mod):
    if name == "ckpt421":
        return model_mod.Muzero.from_arrays(os.path.join(ROOT, "tests", "golden", "weights_ckpt421.npz"))
    with torch.random.fork_rng():
        torch.manual_seed(0)
        return model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=12, action_space_dimensions=9,
                                state_space_dimensions=21, hidden_layer_dimensions=32, number_of_hidden_layer=0, random_tag=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--searches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import stochastic_muzero_amd  # noqa: F401
    mcts_mod, model_mod = (import_module("stochastic-muzero_amd." + m) for m in ("mcts", "model"))
    lines = []
    heads_of = {}
    for name, players, B in SHAPES:
        if name not in heads_of:
            heads_of[name] = net(name, model_mod).heads("cuda:0")
        heads = heads_of[name]
        obs = torch.from_numpy(np.random.RandomState(0).uniform(-0.05, 0.05, (B, heads.desc.obs)).astype(np.float32)).cuda()
        to_play = (torch.arange(B, dtype=torch.int32) % players).cuda()
        for single in (False, True):
            m = mcts_mod.BatchedMCTS(B, num_simulations=a.sims, discount=0.999, root_exploration_fraction=0.1, use_graph=True,
                                     number_of_player=players, players_single_launch=single)
            m.seed(np.arange(B, dtype=np.uint64))
            m.run(obs, heads, train=True, to_play=to_play)
            torch.cuda.synchronize()
            blocks = []
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(a.searches):
                    m.run(obs, heads, train=True, to_play=to_play)
                torch.cuda.synchronize()
                blocks.append((time.perf_counter() - t0) / a.searches)
            ms = 1e3 * float(np.median(blocks))
            rec = dict(net=name, heads=type(heads).__name__, S=heads.S, H=heads.H, L=heads.L, A=heads.A, players=players, trees=B,
                       sims=a.sims, ms_per_search=round(ms, 3), simulations_per_s=round(B * a.sims / (ms * 1e-3)),
                       blocks_ms=[round(1e3 * b, 3) for b in blocks], graph=m._graph is not None, single_launch=m._single is True,
                       kernel=m.engine.last_kernel() if m._single is True else "", device=torch.cuda.get_device_name(0))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            m.engine.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
