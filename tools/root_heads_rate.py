"""The HIP root evaluation of the wide and the large-action mlp_model heads (hip_root=True: smz_mlp_initial_wide / _large, one
launch) against the torch root of the same heads classes (FusedMlpHeads.initial: 12 launches at L = 0, 28 at L = 4), in one run
on one box, both sides packed from the same model.

Shapes (obs, A, S, H, L): config 434 (4,2,61,126,0), checkpoint 450 (4,2,61,126,4) -- wide, Muzero.heads("auto") -- and
(361,362,32,64,1), (4,1024,16,64,1) -- large, Muzero.heads(backend="large"); fresh nets; trees in {256, 1024, 4096}.  Timed:
  root     heads.initial(obs) alone, eager launches
  graph    the 50-simulation step-wise BatchedMCTS search (K = 2, train on, MT19937), graph replays
  single   wide shapes only: the same search with wide_single_launch=True (root evaluation + one search launch)
Per cell either side is built and warmed up (graph capture included) and one more run sizes the blocks; then three rounds, each
timing one block per side in turn (the sides alternate, so a drift of the box hits them alike); a block is as many runs as
fill --window seconds (at least 5), between two synchronisations.  Reported per side: the median block as microseconds per run
and the spread of the three blocks, (max - min) / median; per cell the ratio torch / hip (above 1: the HIP root is faster).
Prints one JSON line per measurement and the table; --out writes both to a file, headed by source_sha16
(bench.kernel_source_sha16: the kernel sources the library was built from).

    python tools/root_heads_rate.py [--nets cfg434,ckpt450,go19,A1024] [--trees 256,1024,4096] [--sims 50] [--window 0.2] [--out FILE]
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

SHAPES = [("cfg434", (4, 2, 61, 126, 0), "auto"), ("ckpt450", (4, 2, 61, 126, 4), "auto"),
          ("go19", (361, 362, 32, 64, 1), "large"), ("A1024", (4, 1024, 16, 64, 1), "large")]


def _blocks(sides, window):
    """sides: dicts with `run`.  Warm-up, sizing run, three alternating rounds -> `blocks` (seconds per run) on every side."""
    for s in sides:
        s["run"]()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s["run"]()
        torch.cuda.synchronize()
        s["n"] = max(5, min(2000, math.ceil(window / max(time.perf_counter() - t0, 1e-6))))
        s["blocks"] = []
    for _ in range(3):
        for s in sides:
            t0 = time.perf_counter()
            for _ in range(s["n"]):
                s["run"]()
            torch.cuda.synchronize()
            s["blocks"].append((time.perf_counter() - t0) / s["n"])


def cell(name, shape, backend, B, sims, window):
    import stochastic_muzero_amd  # noqa: F401
    mcts, model = import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.model")
    obs_dim, A, S, H, L = shape
    torch.manual_seed(0)
    m = model.Muzero(model_structure="mlp_model", observation_space_dimensions=obs_dim, action_space_dimensions=A,
                     state_space_dimensions=S, hidden_layer_dimensions=H, number_of_hidden_layer=L)
    obs = torch.randn(B, obs_dim, generator=torch.Generator().manual_seed(1)).cuda().contiguous()
    heads = {side: m.heads("cuda:0", backend=backend, hip_root=side == "hip") for side in ("torch", "hip")}
    assert type(heads["hip"]) is type(heads["torch"]) and heads["hip"].hip_root and not heads["torch"].hip_root
    out = []
    modes = ["root", "graph"] + (["single"] if backend == "auto" else [])
    for mode in modes:
        sides, engines = [], []
        for side in ("torch", "hip"):
            h = heads[side]
            if mode == "root":
                run = (lambda h=h: h.initial(obs))
            else:
                mc = mcts.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, single_launch=mode == "single",
                                      wide_single_launch=mode == "single", use_graph=mode == "graph")
                mc.seed(np.arange(B, dtype=np.uint64))
                engines.append(mc)
                run = (lambda h=h, mc=mc: mc.run(obs, h, train=True))
            sides.append(dict(side=side, run=run))
        _blocks(sides, window)
        kernel = engines[0].engine.last_kernel().split("<")[0] if engines else ""
        for s in sides:
            t = float(np.median(s["blocks"]))
            out.append(dict(net=name, shape=list(shape), heads=type(heads[s["side"]]).__name__, trees=B, sims=sims, mode=mode,
                            root=s["side"], last_kernel=kernel, runs_per_block=s["n"], us_per_run=round(t * 1e6, 2),
                            spread=round((max(s["blocks"]) - min(s["blocks"])) / t, 4)))
        for mc in engines:
            mc.engine.close()
    return out


def table(recs):
    rows = ["net       trees  mode    torch root us   hip root us   torch / hip   spread torch / hip"]
    cells = {}
    for r in recs:
        cells.setdefault((r["net"], r["trees"], r["mode"]), {})[r["root"]] = r
    for (net, B, mode), c in cells.items():
        rows.append(f'{net:<8}  {B:>5}  {mode:<6}  {c["torch"]["us_per_run"]:>13,.1f}  {c["hip"]["us_per_run"]:>12,.1f}  '
                    f'{c["torch"]["us_per_run"] / c["hip"]["us_per_run"]:>12.2f}   {c["torch"]["spread"]:.3f} / {c["hip"]["spread"]:.3f}')
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default=",".join(n for n, _, _ in SHAPES))
    ap.add_argument("--trees", default="256,1024,4096")
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import bench
    recs = []
    for name, shape, backend in (s for s in SHAPES if s[0] in a.nets.split(",")):
        for B in (int(x) for x in a.trees.split(",") if x):
            for r in cell(name, shape, backend, B, a.sims, a.window):
                recs.append(r)
                print(json.dumps(r), flush=True)
    head = (f"# tools/root_heads_rate.py --sims {a.sims} --window {a.window} ({torch.cuda.get_device_name(0)}; fresh mlp_model nets, K = 2, "
            f"train on, MT19937; us per run, median of three alternating blocks)\n"
            f"# source_sha16 {bench.kernel_source_sha16()}\n")
    text = head + table(recs) + "\n\n" + "\n".join(json.dumps(r) for r in recs) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
