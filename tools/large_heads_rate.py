"""Search rate with the large-action HIP heads (heads.HipMlpLargeHeads, Muzero.heads(backend="large")) against the torch-GEMM
heads (backend="torch", FusedMlpHeads) on the same step-wise BatchedMCTS graph, in one run on one box.

Fresh mlp_model nets (obs 6, S 16, H 64, L 1), K = 2, 50 simulations, train=True, graph replays; A in {64, 100, 256, 362, 1024}
x trees in {256, 1024, 4096} x {MT19937, Philox}.  At A = 64 and 100 backend="auto" (HipMlpTileHeads, the wide tile kernel on
the one-hot input) is timed too.  Per cell every backend builds its search and runs one warm-up search (which captures the
graph) and one more to size the blocks; then three rounds, each timing one block per backend in turn (the backends alternate,
so a drift of the box hits them alike); a block is as many searches as fill --window seconds (at least 5), between two
synchronisations.  --mode single times two searches with the SAME large-action heads instead: the step-wise graph replay
("graph") against BatchedMCTS(large_single_launch=True) ("single": the heads' root evaluation, the root kernels and one
smz_search_mlp_large launch for all rounds), by the same method; its table gives ms per search of both and single / graph as a
rate ratio (below 1: the single launch loses); --trees-per-wg 1,2 adds the single launch with SMZ_LARGE_SEARCH_T = 1 and 2 (trees per
workgroup, an A/B of the launch geometry; the search does not depend on it).  Reported per backend: the median block as simulations/s and ms per search, and
the spread of the three blocks, (max - min) / median.  Prints one JSON line per measurement and the table; --out writes both to a file, headed by
source_sha16 (bench.kernel_source_sha16: the kernel sources the library was built from).

    python tools/large_heads_rate.py [--mode heads|single] [--actions 64,100,256,362,1024] [--trees 256,1024,4096] [--sims 50]
                                     [--window 0.25] [--out FILE]
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


def _env(side_env):
    """The environment of one side's searches (libsmz reads SMZ_LARGE_SEARCH_T on every call)."""
    for k, v in side_env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def cell(A, B, sims, rng, window, mode="heads", per_wg=()):
    import stochastic_muzero_amd  # noqa: F401
    mcts, model = import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.model")
    torch.manual_seed(0)
    m = model.Muzero(model_structure="mlp_model", observation_space_dimensions=6, action_space_dimensions=A,
                     state_space_dimensions=16, hidden_layer_dimensions=64, number_of_hidden_layer=1)
    obs = torch.randn(B, 6, generator=torch.Generator().manual_seed(1)).cuda()
    sides = []
    if mode == "single":            # (side name, heads backend, BatchedMCTS switches)
        plan = [("graph", "large", dict(single_launch=False), None), ("single", "large", dict(large_single_launch=True), None)]
        plan += [(f"single_T{t}", "large", dict(large_single_launch=True), str(t)) for t in per_wg]
    else:
        plan = [(b, b, dict(single_launch=False), None) for b in ("large", "torch") + (("auto",) if A + 16 <= 128 else ())]
    for backend, heads_backend, kw, trees_per_wg in plan:
        heads = m.heads("cuda:0", backend=heads_backend)
        env = dict(SMZ_LARGE_SEARCH_T=trees_per_wg)
        _env(env)
        mc = mcts.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, rng_mode=rng, **kw)
        mc.seed(np.arange(B, dtype=np.uint64))
        mc.run(obs, heads, train=True)                  # warm-up: allocator, GEMM algorithms, graph capture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mc.run(obs, heads, train=True)
        torch.cuda.synchronize()
        n = max(5, min(400, math.ceil(window / max(time.perf_counter() - t0, 1e-5))))
        sides.append(dict(backend=backend, heads=heads, mc=mc, n=n, blocks=[], env=env))
    for _ in range(3):
        for s in sides:
            _env(s["env"])
            t0 = time.perf_counter()
            for _ in range(s["n"]):
                s["mc"].run(obs, s["heads"], train=True)
            torch.cuda.synchronize()
            s["blocks"].append((time.perf_counter() - t0) / s["n"])
    out = []
    for s in sides:
        t = float(np.median(s["blocks"]))
        out.append(dict(actions=A, trees=B, sims=sims, K=2, rng=rng, backend=s["backend"], heads=type(s["heads"]).__name__,
                        graph=s["mc"]._graph is not None, large_actions=bool(s["mc"].engine.large_actions),
                        last_kernel=s["mc"].engine.last_kernel(),
                        searches_per_block=s["n"], ms_per_search=round(t * 1e3, 4), simulations_per_s=round(B * sims / t),
                        spread=round((max(s["blocks"]) - min(s["blocks"])) / t, 4)))
        s["mc"].engine.close()
    _env(dict(SMZ_LARGE_SEARCH_T=None))
    return out


def table(recs):
    rows = ["actions  trees  rng      large sims/s   torch sims/s  large/torch   auto (wide tile) sims/s   spread large / torch"]
    cells = {}
    for r in recs:
        cells.setdefault((r["actions"], r["trees"], r["rng"]), {})[r["backend"]] = r
    for (A, B, rng), c in cells.items():
        auto = f'{c["auto"]["simulations_per_s"]:>12,}' if "auto" in c else " " * 11 + "-"
        rows.append(f'{A:>7}  {B:>5}  {rng:<7}  {c["large"]["simulations_per_s"]:>12,}   {c["torch"]["simulations_per_s"]:>12,}  '
                    f'{c["large"]["simulations_per_s"] / c["torch"]["simulations_per_s"]:>11.2f}   {auto:>23}   '
                    f'{c["large"]["spread"]:.3f} / {c["torch"]["spread"]:.3f}')
    return "\n".join(rows)


def table_single(recs):
    rows = ["actions  trees  rng      graph ms/search  single ms/search   graph sims/s  single sims/s  single/graph   spread graph / single"]
    cells = {}
    for r in recs:
        cells.setdefault((r["actions"], r["trees"], r["rng"]), {})[r["backend"]] = r
    for (A, B, rng), c in cells.items():
        g, s = c["graph"], c["single"]
        extra = "".join(f'   {k[7:]}: {v["ms_per_search"]:.3f} ms' for k, v in c.items() if k.startswith("single_T"))
        rows.append(f'{A:>7}  {B:>5}  {rng:<7}  {g["ms_per_search"]:>15.3f}  {s["ms_per_search"]:>16.3f}   {g["simulations_per_s"]:>12,}  '
                    f'{s["simulations_per_s"]:>13,}  {s["simulations_per_s"] / g["simulations_per_s"]:>12.2f}   '
                    f'{g["spread"]:.3f} / {s["spread"]:.3f}{extra}')
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actions", default="64,100,256,362,1024")
    ap.add_argument("--trees", default="256,1024,4096")
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--mode", choices=("heads", "single"), default="heads")
    ap.add_argument("--trees-per-wg", default="", help="--mode single: also time the single launch with SMZ_LARGE_SEARCH_T = each of these")
    ap.add_argument("--out")
    a = ap.parse_args()
    import bench
    recs = []
    for A in (int(x) for x in a.actions.split(",") if x):
        for B in (int(x) for x in a.trees.split(",") if x):
            for rng in ("mt19937", "philox"):
                for r in cell(A, B, a.sims, rng, a.window, a.mode, [int(x) for x in a.trees_per_wg.split(",") if x]):
                    recs.append(r)
                    print(json.dumps(r), flush=True)
    what = ("step-wise graph replay against large_single_launch=True, the same large-action heads" if a.mode == "single"
            else "step-wise graph replays")
    head = (f"# tools/large_heads_rate.py{' --mode single' if a.mode == 'single' else ''}{' --trees-per-wg ' + a.trees_per_wg if a.trees_per_wg else ''} --actions {a.actions} --trees {a.trees} "
            f"--sims {a.sims} --window {a.window} ({torch.cuda.get_device_name(0)}; fresh mlp_model nets obs 6 / S 16 / "
            f"H 64 / L 1, K = 2, train on, {what}; median of three alternating blocks)\n"
            f"# source_sha16 {bench.kernel_source_sha16()}\n")
    text = head + (table_single if a.mode == "single" else table)(recs) + "\n\n" + "\n".join(json.dumps(r) for r in recs) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
