"""Golden vectors of searches with more than 32 actions (the large-action handles), written by the reference itself.

TEST INFRASTRUCTURE.  Builds on oracle/gen_golden.py (run_case, TapeModel, CraftedModel, fresh_mlp, post_search) and imports the
reference through oracle/_ref_import.py, as tools/gen_golden_players.py does, so it runs only where the reference is available
(SMZ_REFERENCE_DIR).  Each fixture holds a few taped searches of the reference's own Monte_carlo_tree_search with a fresh
Discrete(A) mlp_model (small trunks: the fixtures stay small), and the act outputs at every temperature (post_search).  The GPU
tests read the committed fixtures under tests/golden/large_actions/ and nothing else.

    python tools/gen_golden_large_actions.py [NAME ...]      (no name: every fixture; names, of new_fixtures' entries: only those,
                                                              every other file stays as it is)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import _ref_import as R  # noqa: E402
import gen_golden as G  # noqa: E402
import gen_golden_players as GP  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "large_actions")
OBS = 4


def _obs(n, seed):
    return [torch.tensor(np.random.RandomState(seed + s).uniform(-0.5, 0.5, (1, OBS)).astype(np.float32)) for s in range(n)]


def cases(ref, model, A, K, sims, train, n, seed, **extra):
    kw = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
              maxium_action_sample=K, num_simulations=sims, number_of_player=1, custom_loop=None)
    kw.update(extra)
    out = [G.run_case(ref, model, o, seed + s, kw, train=train, obs_dim=OBS) for s, o in enumerate(_obs(n, 7000 + seed))]
    return kw, out


ONLY = set(sys.argv[1:])


def save(name, kw, recs):
    data = G.stack_cases(recs)
    for k, v in kw.items():
        if v is not None:
            data["cfg_" + k] = np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB, {len(recs)} cases)")


def main():
    os.makedirs(OUT, exist_ok=True)
    ref = R.import_reference()
    torch.set_num_threads(1)
    net = lambda A, seed: G.fresh_mlp(ref, OBS, A, S=8, H=16, L=0, seed=seed)   # noqa: E731
    if ONLY:
        return new_fixtures(ref, net)
    save("la_A33_K2_sims50", *cases(ref, net(33, 1), 33, 2, 50, True, 2, 100))            # the first LA-only width
    save("la_A64_K2_sims50_notrain", *cases(ref, net(64, 2), 64, 2, 50, False, 2, 200))
    save("la_A100_K5_sims30", *cases(ref, net(100, 3), 100, 5, 30, True, 2, 300))
    save("la_A129_K3_sims30", *cases(ref, net(129, 4), 129, 3, 30, True, 2, 400))        # above numpy's 128-element block
    save("la_A256_K256_sims10", *cases(ref, net(256, 5), 256, 256, 10, True, 2, 500))     # interior nodes as wide as the root
    save("la_A1000_K2_sims20", *cases(ref, net(1000, 6), 1000, 2, 20, True, 4, 600))
    crafted = G.CraftedModel(256, 8, np.full(256, 1.0 / 256, np.float32))                 # constant policy: ucb ties
    save("la_A256_K2_sims30_crafted", *cases(ref, crafted, 256, 2, 30, True, 2, 700))
    # two players (the root player of each case as tools/gen_golden_players.py records it)
    kw = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
              maxium_action_sample=2, num_simulations=30, number_of_player=2, custom_loop=None)
    GP.save.__globals__["OUT"] = OUT
    GP.save("la_A64_K2_sims30_p2", kw, GP.search_cases(ref, net(64, 8), _obs(1, 7800), kw, roots=(0, 1)))
    new_fixtures(ref, net)


def new_fixtures(ref, net):
    """The fixtures added with the oracle's 1024-action range (each is skipped unless named when names are given)."""
    todo = [("la_A1024_K3_sims12", lambda: cases(ref, net(1024, 9), 1024, 3, 12, True, 2, 800)),        # the action limit
            ("la_A200_K200_sims12", lambda: cases(ref, net(200, 10), 200, 200, 12, True, 2, 900)),      # K > 128: ragged 96 + 104 split
            ("la_A129_K3_sims12_alpha1", lambda: cases(ref, net(129, 11), 129, 3, 12, True, 2, 1000,    # gamma(1): two words a round
                                                       root_dirichlet_alpha=1.0))]
    for name, make in todo:
        if not ONLY or name in ONLY:
            save(name, *make())


if __name__ == "__main__":
    main()
