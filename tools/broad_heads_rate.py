"""Search rate with the broad HIP heads (heads.HipMlpBroadHeads, Muzero.heads(backend="broad")) against the heads "auto" picks
for the same fresh net (FusedMlpHeads, the torch GEMMs: these shapes are outside every older HIP layout) on the same step-wise
BatchedMCTS graph, in one run on one box.  --backends chooses the sides: the first one is measured against each of the others
(--backends broad_bf16,broad,auto: the bf16 broad heads, heads.HipMlpBroadBf16Heads, against both).

Fresh mlp_model nets (obs 6, L 1), K = 2, 50 simulations, MT19937, train=True, graph replays; H in {256, 512} x S in {64, 128} x
A in {4, 64} x trees in {256, 1024, 4096}.  Per cell both backends build their search and run one warm-up search (which captures
the graph) and one more to size the blocks; then three rounds, each timing one block per backend in turn (the backends
alternate, so a drift of the box hits them alike); a block is as many searches as fill --window seconds (at least 5), between
two synchronisations.  Reported per backend: the median block as simulations/s and ms per search, and the spread of the three
blocks, (max - min) / median.  Prints one JSON line per measurement and the table; --out writes both to a file, headed by
source_sha16 (bench.kernel_source_sha16: the kernel sources the library was built from).

    python tools/broad_heads_rate.py [--hidden 256,512] [--state 64,128] [--actions 4,64] [--trees 256,1024,4096] [--sims 50]
                                     [--window 0.25] [--backends broad,auto] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time
from importlib import import_module

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


HEADS = {"broad": "HipMlpBroadHeads", "broad_bf16": "HipMlpBroadBf16Heads", "auto": "FusedMlpHeads"}


def cell(H, S, A, B, sims, window, backends=("broad", "auto")):
    import stochastic_muzero_amd  # noqa: F401
    mcts, model = import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.model")
    torch.manual_seed(0)
    m = model.Muzero(model_structure="mlp_model", observation_space_dimensions=6, action_space_dimensions=A,
                     state_space_dimensions=S, hidden_layer_dimensions=H, number_of_hidden_layer=1)
    obs = torch.randn(B, 6, generator=torch.Generator().manual_seed(1)).cuda()
    sides = []
    for backend in backends:
        heads = m.heads("cuda:0", backend=backend)
        mc = mcts.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, rng_mode="mt19937", single_launch=False)
        mc.seed(np.arange(B, dtype=np.uint64))
        mc.run(obs, heads, train=True)                  # warm-up: allocator, GEMM algorithms, graph capture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mc.run(obs, heads, train=True)
        torch.cuda.synchronize()
        n = max(5, min(400, math.ceil(window / max(time.perf_counter() - t0, 1e-5))))
        sides.append(dict(backend=backend, heads=heads, mc=mc, n=n, blocks=[]))
    for _ in range(3):
        for s in sides:
            t0 = time.perf_counter()
            for _ in range(s["n"]):
                s["mc"].run(obs, s["heads"], train=True)
            torch.cuda.synchronize()
            s["blocks"].append((time.perf_counter() - t0) / s["n"])
    out = []
    for s in sides:
        t = float(np.median(s["blocks"]))
        out.append(dict(hidden=H, state=S, actions=A, trees=B, sims=sims, K=2, rng="mt19937", backend=s["backend"],
                        heads=type(s["heads"]).__name__, graph=s["mc"]._graph is not None,
                        large_actions=bool(s["mc"].engine.large_actions), searches_per_block=s["n"],
                        ms_per_search=round(t * 1e3, 4), simulations_per_s=round(B * sims / t),
                        spread=round((max(s["blocks"]) - min(s["blocks"])) / t, 4)))
        s["mc"].engine.close()
    return out


def table(recs):
    names = list(dict.fromkeys(r["backend"] for r in recs))
    first, others = names[0], names[1:]
    label = lambda n: "auto (torch)" if n == "auto" else n
    rows = ["     H    S  actions  trees  " + "  ".join(f"{label(n) + ' sims/s':>20}" for n in names) + "  " +
            "  ".join(f"{first + '/' + n:>16}" for n in others) + "  " + "  ".join(f"{label(n) + ' ms/search':>22}" for n in names) +
            "   spread " + " / ".join(names)]
    cells = {}
    for r in recs:
        cells.setdefault((r["hidden"], r["state"], r["actions"], r["trees"]), {})[r["backend"]] = r
    for (H, S, A, B), c in cells.items():
        rows.append(f'{H:>6}  {S:>3}  {A:>7}  {B:>5}  ' + "  ".join(f'{c[n]["simulations_per_s"]:>20,}' for n in names) + "  " +
                    "  ".join(f'{c[first]["simulations_per_s"] / c[n]["simulations_per_s"]:>16.2f}' for n in others) + "  " +
                    "  ".join(f'{c[n]["ms_per_search"]:>22.3f}' for n in names) + "   " + " / ".join(f'{c[n]["spread"]:.3f}' for n in names))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", default="256,512")
    ap.add_argument("--state", default="64,128")
    ap.add_argument("--actions", default="4,64")
    ap.add_argument("--trees", default="256,1024,4096")
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--backends", default="broad,auto")
    ap.add_argument("--out")
    a = ap.parse_args()
    import bench
    ints = lambda s: [int(x) for x in s.split(",") if x]
    backends = [b for b in a.backends.split(",") if b]
    assert len(backends) >= 2 and set(backends) <= set(HEADS), backends
    recs = []
    for H in ints(a.hidden):
        for S in ints(a.state):
            for A in ints(a.actions):
                for B in ints(a.trees):
                    for r in cell(H, S, A, B, a.sims, a.window, backends):
                        assert r["heads"] == HEADS[r["backend"]], r
                        recs.append(r)
                        print(json.dumps(r), flush=True)
    head = (f"# tools/broad_heads_rate.py --hidden {a.hidden} --state {a.state} --actions {a.actions} --trees {a.trees} --sims {a.sims} "
            f"--window {a.window} --backends {a.backends} ({torch.cuda.get_device_name(0)}; fresh mlp_model nets obs 6 / L 1, K = 2, MT19937, train on, "
            f"step-wise graph replays; median of three alternating blocks)\n"
            f"# source_sha16 {bench.kernel_source_sha16()}\n")
    text = head + table(recs) + "\n\n" + "\n".join(json.dumps(r) for r in recs) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
