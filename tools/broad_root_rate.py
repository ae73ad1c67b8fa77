"""The HIP root evaluation of the broad mlp_model heads (hip_root=True: smz_mlp_initial_broad, one launch) against the torch root
of the same heads classes (FusedMlpHeads.initial: 16 launches at L = 1), in one run on one box, both sides packed from the same
model.  The bf16 heads run the same float32 root kernel on a float32 image of their own; their searches are shorter, so the
root's share of one is larger.

Fresh mlp_model nets (obs 6, L 1), the grid of tools/broad_heads_rate.py: H in {256, 512} x S in {64, 128} x A in {4, 64} x trees in
{256, 1024, 4096}, backends broad and broad_bf16.  Timed:
  root     heads.initial(obs) alone, eager launches
  graph    the 50-simulation step-wise BatchedMCTS search (K = 2, train on, MT19937), graph replays
Per cell either side is built and warmed up (graph capture included) and one more run sizes the blocks; then three rounds, each
timing one block per side in turn (the sides alternate, so a drift of the box hits them alike); a block is as many runs as
fill --window seconds (at least 5), between two synchronisations.  Reported per side: the median block as microseconds per run
and the spread of the three blocks, (max - min) / median; per cell the ratio torch / hip (above 1: the HIP root is faster).
Prints one JSON line per measurement and the table; --out writes both to a file, headed by source_sha16
(bench.kernel_source_sha16: the kernel sources the library was built from).

    python tools/broad_root_rate.py [--hidden 256,512] [--state 64,128] [--actions 4,64] [--trees 256,1024,4096]
                                    [--backends broad,broad_bf16] [--sims 50] [--window 0.2] [--out FILE]
"""
import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from root_heads_rate import _blocks  # noqa: E402

HEADS = {"broad": "HipMlpBroadHeads", "broad_bf16": "HipMlpBroadBf16Heads"}


def cell(backend, H, S, A, B, sims, window):
    import stochastic_muzero_amd  # noqa: F401
    mcts, model = import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.model")
    torch.manual_seed(0)
    m = model.Muzero(model_structure="mlp_model", observation_space_dimensions=6, action_space_dimensions=A,
                     state_space_dimensions=S, hidden_layer_dimensions=H, number_of_hidden_layer=1)
    obs = torch.randn(B, 6, generator=torch.Generator().manual_seed(1)).cuda().contiguous()
    heads = {side: m.heads("cuda:0", backend=backend, hip_root=side == "hip") for side in ("torch", "hip")}
    assert type(heads["hip"]) is type(heads["torch"]) and type(heads["hip"]).__name__ == HEADS[backend]
    assert heads["hip"].hip_root and "initial" in vars(heads["hip"]) and "initial" not in vars(heads["torch"])
    out = []
    for mode in ("root", "graph"):
        sides, engines = [], []
        for side in ("torch", "hip"):
            h = heads[side]
            if mode == "root":
                run = (lambda h=h: h.initial(obs))
            else:
                mc = mcts.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, rng_mode="mt19937", single_launch=False,
                                      use_graph=True)
                mc.seed(np.arange(B, dtype=np.uint64))
                engines.append(mc)
                run = (lambda h=h, mc=mc: mc.run(obs, h, train=True))
            sides.append(dict(side=side, run=run))
        _blocks(sides, window)
        assert all(mc._graph is not None for mc in engines)
        for s in sides:
            t = float(np.median(s["blocks"]))
            out.append(dict(backend=backend, hidden=H, state=S, actions=A, heads=HEADS[backend], trees=B, sims=sims, mode=mode,
                            root=s["side"], runs_per_block=s["n"], us_per_run=round(t * 1e6, 2),
                            spread=round((max(s["blocks"]) - min(s["blocks"])) / t, 4)))
        for mc in engines:
            mc.engine.close()
    return out


def table(recs):
    rows = ["backend       H    S    A  trees  mode    torch root us   hip root us   torch / hip   spread torch / hip"]
    cells = {}
    for r in recs:
        cells.setdefault((r["backend"], r["hidden"], r["state"], r["actions"], r["trees"], r["mode"]), {})[r["root"]] = r
    for (backend, H, S, A, B, mode), c in cells.items():
        rows.append(f'{backend:<10}  {H:>4}  {S:>3}  {A:>3}  {B:>5}  {mode:<6}  {c["torch"]["us_per_run"]:>13,.1f}  '
                    f'{c["hip"]["us_per_run"]:>12,.1f}  {c["torch"]["us_per_run"] / c["hip"]["us_per_run"]:>12.3f}   '
                    f'{c["torch"]["spread"]:.3f} / {c["hip"]["spread"]:.3f}')
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", default="256,512")
    ap.add_argument("--state", default="64,128")
    ap.add_argument("--actions", default="4,64")
    ap.add_argument("--trees", default="256,1024,4096")
    ap.add_argument("--backends", default="broad,broad_bf16")
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import bench
    ints = lambda s: [int(x) for x in s.split(",") if x]
    backends = [b for b in a.backends.split(",") if b]
    assert backends and set(backends) <= set(HEADS), backends
    recs = []
    for backend in backends:
        for H in ints(a.hidden):
            for S in ints(a.state):
                for A in ints(a.actions):
                    for B in ints(a.trees):
                        for r in cell(backend, H, S, A, B, a.sims, a.window):
                            recs.append(r)
                            print(json.dumps(r), flush=True)
    head = (f"# tools/broad_root_rate.py --hidden {a.hidden} --state {a.state} --actions {a.actions} --trees {a.trees} --backends {a.backends} "
            f"--sims {a.sims} --window {a.window} ({torch.cuda.get_device_name(0)}; fresh mlp_model nets obs 6 / L 1, K = 2, train on, MT19937; "
            f"us per run, median of three alternating blocks)\n"
            f"# source_sha16 {bench.kernel_source_sha16()}\n")
    text = head + table(recs) + "\n\n" + "\n".join(json.dumps(r) for r in recs) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
