"""Search rate of the wide mlp_model shapes (HipMlpTileHeads): the step-wise graph path against the single launch.

The reference's checkpoint-450 net (S 61, H 126, L 4) and the config-434-shaped net (S 61, H 126, L 0) of
tests/golden/weights_*.npz, 4096 and 1024 trees x 50 simulations, train=True.  Per net and size, in the same call and with the
same heads: the step-wise search replayed as one HIP graph, and BatchedMCTS(wide_single_launch=True) (the heads' root
evaluation + one smz_search_mlp_wide launch per search).  Each: one warm-up search, then three blocks of `--searches` searches
between synchronisations; the median block is reported.  Prints one JSON line per measurement and, with --out, appends the same
lines to a file.

    python tools/wide_rate.py [--trees 4096 1024] [--sims 50] [--searches 10] [--out FILE]
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
NETS = (("ckpt450", "weights_ckpt450.npz"), ("cfg434shape", "weights_cfg434shape.npz"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, nargs="+", default=[4096, 1024])
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--searches", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import stochastic_muzero_amd  # noqa: F401
    mcts_mod, model_mod = (import_module("stochastic-muzero_amd." + m) for m in ("mcts", "model"))
    lines = []
    for net, wfile in NETS:
        model = model_mod.Muzero.from_arrays(os.path.join(ROOT, "tests", "golden", wfile))
        heads = model.heads("cuda:0")
        for B in a.trees:
            obs = torch.from_numpy(np.random.RandomState(0).uniform(-0.05, 0.05, (B, 4)).astype(np.float32)).cuda()
            for single in (False, True):
                m = mcts_mod.BatchedMCTS(B, num_simulations=a.sims, discount=0.999, root_exploration_fraction=0.1, use_graph=True,
                                         wide_single_launch=single)
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
                rec = dict(net=net, heads=type(heads).__name__, S=heads.S, H=heads.H, L=heads.L, trees=B, sims=a.sims,
                           ms_per_search=round(ms, 3), simulations_per_s=round(B * a.sims / (ms * 1e-3)),
                           graph=m._graph is not None, single_launch=m._single is True,
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
