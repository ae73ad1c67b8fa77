"""Search rate of the lstm_model family: step-wise BatchedMCTS searches with HipLstmHeads against LstmTorchHeads.

The CartPole-shaped reference net of tests/golden/lstm/lstmnet_cartpole_L1.npz (obs 4, A 2, S 31, H 64, L 1), 50
simulations, train=True, graph replays.  Each backend: one warm-up search (captures the graph), then three blocks of
`--searches` searches between synchronisations; the median block is reported.  Prints one JSON line per backend and, with
--out, appends the same lines to a file.

    python tools/lstm_rate.py [--trees 4096] [--sims 50] [--searches 10] [--out FILE] [--single-launch]

--single-launch: the pair measured is the step-wise graph path with HipLstmHeads (as above) and the single launch
(BatchedMCTS(lstm_single_launch=True): smz_lstm_initial + one smz_search_lstm launch per search), in the same call; the torch
backend is left out.
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
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--searches", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--single-launch", action="store_true")
    a = ap.parse_args()
    import stochastic_muzero_amd  # noqa: F401
    mcts_mod, model_mod = (import_module("stochastic-muzero_amd." + m) for m in ("mcts", "model"))
    model = model_mod.Muzero.from_state_dicts(os.path.join(ROOT, "tests", "golden", "lstm", "lstmnet_cartpole_L1.npz"))
    B = a.trees
    obs = torch.from_numpy(np.random.RandomState(0).uniform(-0.05, 0.05, (B, 4)).astype(np.float32)).cuda()
    lines = []
    runs = (("hip", False), ("hip", True)) if a.single_launch else (("hip", False), ("torch", False))
    for backend, single in runs:
        heads = model.heads("cuda:0", backend=backend)
        m = mcts_mod.BatchedMCTS(B, num_simulations=a.sims, discount=0.999, root_exploration_fraction=0.1, use_graph=True,
                                 lstm_single_launch=single)
        m.seed(np.arange(B, dtype=np.uint64))
        m.run(obs, heads, train=True)
        torch.cuda.synchronize()
        blocks = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(a.searches):
                m.run(obs, heads, train=True)
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t0) / a.searches)
        ms = 1e3 * float(np.median(blocks))
        rec = dict(backend=backend, heads=type(heads).__name__, trees=B, sims=a.sims, ms_per_search=round(ms, 3),
                   simulations_per_s=round(B * a.sims / (ms * 1e-3)), graph=m._graph is not None,
                   single_launch=m._single is True, kernel=m.engine.last_kernel() if m._single is True else "",
                   device=torch.cuda.get_device_name(0))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
