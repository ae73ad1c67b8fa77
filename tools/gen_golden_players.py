"""Golden vectors of multi-player searches (number_of_player > 1, custom_loop), written by the reference itself.

TEST INFRASTRUCTURE.  Builds on oracle/gen_golden.py (run_case, gen_selfplay, TapeModel, load_ckpt, fresh_mlp) and imports
the reference through oracle/_ref_import.py, so it runs only where the reference is available (SMZ_REFERENCE_DIR).  The GPU
tests read the committed fixtures under tests/golden/players/ and nothing else.

Per search case, beside run_case's fields:
  root_to_play  the root's player index (the reference's Player_cycle.global_count is set before run())
  tree_to_play  every node's `to_play`, node ids in creation order (root 0, its children 1..A, then K per expansion)
and the cycle config as cfg_number_of_player / cfg_custom_loop.  The game fixture is the reference's own play_game with two
players (gen_selfplay's shape), plus the root player of every step.

    python tools/gen_golden_players.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _ref_import as R  # noqa: E402
import gen_golden as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "players")


class _Rooted:
    """Factory for a Monte_carlo_tree_search subclass whose searches start at a chosen root player and keep their root."""

    def __init__(self, base):
        rooted = self

        class Search(base):
            def run(self, *args, **kwargs):
                if rooted.root_to_play is not None:
                    self.cycle.global_count = rooted.root_to_play
                rooted.roots.append(int(self.cycle.global_count))
                root = super().run(*args, **kwargs)
                rooted.last = root
                return root

        self.cls, self.root_to_play, self.roots, self.last = Search, None, [], None


def tree_to_play(root, child_base, n):
    out = np.full(n, -1, np.int32)
    stack = [(root, 0)]
    while stack:
        node, i = stack.pop()
        out[i] = int(node.to_play)
        for j, c in enumerate(node.children.values()):
            stack.append((c, int(child_base[i]) + j))
    assert (out >= 0).all()
    return out


def search_cases(ref, model, obs_list, kw, roots):
    base = ref.mcts.Monte_carlo_tree_search
    rooted = _Rooted(base)
    ref.mcts.Monte_carlo_tree_search = rooted.cls
    cases = []
    try:
        for r in roots:
            for s, obs in enumerate(obs_list):
                rooted.root_to_play = r
                seed = 10 * r + s
                rec = G.run_case(ref, model, obs, seed, kw)
                rec["root_to_play"] = np.int32(r)
                rec["tree_to_play"] = tree_to_play(rooted.last, rec["tree_child_base"], rec["tree_visit"].size)
                cases.append(rec)
    finally:
        ref.mcts.Monte_carlo_tree_search = base
    return cases


def save(name, kw, cases):
    data = G.stack_cases(cases)
    for k, v in kw.items():
        if v is not None:
            data["cfg_" + k] = np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB, {len(cases)} cases)")


def gen_game(ref, mz, name, players, sims, temperature, limit, seed):
    """gen_selfplay (the reference's play_game over the stand-in CartPole) with `players` players."""
    base = ref.mcts.Monte_carlo_tree_search
    rooted = _Rooted(base)

    class Players(rooted.cls):
        def __init__(self, **kw):
            super().__init__(**dict(kw, number_of_player=players))

    ref.mcts.Monte_carlo_tree_search = Players
    G.OUT, out0 = OUT, G.OUT
    try:
        G.gen_selfplay(ref, mz, name, sims=sims, temperature=temperature, limit=limit, seed=seed)
    finally:
        ref.mcts.Monte_carlo_tree_search = base
        G.OUT = out0
    path = os.path.join(OUT, name + ".npz")
    z = dict(np.load(path))
    z["cfg_number_of_player"] = np.asarray(players)
    z["root_to_play"] = np.array(rooted.roots, np.int32)
    np.savez_compressed(path, **z)


def main():
    os.makedirs(OUT, exist_ok=True)
    ref = R.import_reference()
    torch.set_num_threads(1)
    base = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.999, root_dirichlet_alpha=0.25,
                root_exploration_fraction=0.1, maxium_action_sample=2, number_of_player=1, custom_loop=None)
    mz = G.load_ckpt(ref, 421)
    anchor = torch.tensor([[0.01, -0.02, 0.03, 0.04]])
    other = torch.tensor(np.random.RandomState(4000).uniform(-0.05, 0.05, (1, 4)).astype(np.float32))
    obs = [anchor, other]
    kw = dict(base, num_simulations=50, number_of_player=2)
    save("ckpt421_p2_sims50", kw, search_cases(ref, mz, obs, kw, roots=(0, 1)))
    kw = dict(base, num_simulations=100, number_of_player=3)
    save("ckpt421_p3_sims100", kw, search_cases(ref, mz, obs, kw, roots=(0, 1, 2)))
    kw = dict(base, num_simulations=50, custom_loop="1>2>1>3")
    save("ckpt421_loop1213_sims50", kw, search_cases(ref, mz, obs, kw, roots=(0, 1, 2, 3)))
    ll = G.fresh_mlp(ref, 8, 4, L=0, seed=0)            # tests/golden/weights_lunar_L0.npz
    kw = dict(base, num_simulations=30, maxium_action_sample=4, custom_loop="1>1>2")
    lobs = [torch.tensor(np.random.RandomState(4100 + s).randn(1, 8).astype(np.float32)) for s in range(2)]
    save("lunar_K4_loop112_sims30", kw, search_cases(ref, ll, lobs, kw, roots=(0, 1, 2)))
    gen_game(ref, mz, "selfplay421_p2_sims10_T1", players=2, sims=10, temperature=1.0, limit=24, seed=5)


if __name__ == "__main__":
    main()
