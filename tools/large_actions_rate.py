"""Search rate of the large-action (wave-per-tree) tree kernels: step-wise searches of BatchedMCTS with a fresh mlp_model's
heads (obs 6, S 16, H 64, L 1; HipMlpHeads while A + S <= 128, the torch heads above), K = 2, MT19937, train=True, graph
replays.  Per action count: one warm-up search (captures the graph), then three blocks of `--searches` searches between
synchronisations; the median block is reported.  --compare32 adds A = 32 on the per-lane kernels (smz_create) against the same
search on a large-action handle.  Prints one JSON line per configuration and, with --out, appends the lines to a file.

    python tools/large_actions_rate.py [--trees 4096] [--sims 50] [--searches 5] [--actions 33,64,100,256,1000]
                                       [--compare32] [--out FILE]
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


def rate(A, B, sims, searches, large=None):
    import stochastic_muzero_amd  # noqa: F401
    mcts, model = import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.model")
    torch.manual_seed(0)
    m = model.Muzero(model_structure="mlp_model", observation_space_dimensions=6, action_space_dimensions=A,
                     state_space_dimensions=16, hidden_layer_dimensions=64, number_of_hidden_layer=1)
    heads = m.heads("cuda:0")
    mc = mcts.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, single_launch=False, rng_mode="mt19937")
    if large is not None:                     # (A = 32 comparison: force the handle kind)
        mc._ensure_engine(A, 16)
        eng = mc.engine
        if eng.large_actions != large:
            eng.close()
            mc.engine = import_module("stochastic-muzero_amd.engine").SearchEngine(
                B, A, 16, device=mc.device, rng_mode=mc.rng_mode, large_actions=large, **mc._engine_kwargs())
    obs = torch.randn(B, 6, generator=torch.Generator().manual_seed(1)).cuda()
    mc.run(obs, heads, train=True)
    torch.cuda.synchronize()
    blocks = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(searches):
            mc.run(obs, heads, train=True)
        torch.cuda.synchronize()
        blocks.append(time.perf_counter() - t0)
    t = sorted(blocks)[1] / searches
    return dict(actions=A, trees=B, sims=sims, K=2, rng="mt19937", large_actions=bool(mc.engine.large_actions),
                heads=type(heads).__name__, ms_per_search=t * 1e3, simulations_per_s=B * sims / t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--searches", type=int, default=5)
    ap.add_argument("--actions", default="33,64,100,256,1000")
    ap.add_argument("--compare32", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    runs = [(int(x), None) for x in a.actions.split(",") if x]
    if a.compare32:
        runs += [(32, False), (32, True)]
    for A, large in runs:
        line = json.dumps(rate(A, a.trees, a.sims, a.searches, large))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
