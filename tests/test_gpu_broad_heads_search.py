"""Step-wise searches whose recurrent networks are the broad HIP heads (heads.HipMlpBroadHeads, Muzero.heads(backend="broad")):
a round is three launches -- select, smz_mlp_recurrent_broad, expand + backup -- on a per-lane handle (A = 4) and on a
large-action handle (A = 129); the root is FusedMlpHeads.initial, on the torch GEMMs.

The method is that of tests/test_gpu_large_heads_search.py (_Recording / _Tape, imported from there): the recorded head outputs
of every round are replayed as a tape on a second engine, which must build the same trees and leave the same stream positions
bit for bit (expand consumed exactly what the heads wrote, in the rows select named), and every round's head outputs must be
the float64 restatement's on that round's parent rows, actions and branches (select handed the heads the rows they read).
The captured graph (smz_mlp_recurrent_broad inside it) must give the trees of the eager run."""
import numpy as np
import pytest
import torch

import mlp_reference as mr
from search_helpers import _pkg
from test_gpu_large_actions import _streams_equal, _trees_equal
from test_gpu_large_heads_search import GAIN, _obs, _Recording, _rounds_match_the_restatement, _search, _Tape

pytestmark = pytest.mark.gpu

# (shape (obs, A, S, H, L), trees, simulations, K, large-action handle)
CASES = [((4, 4, 70, 200, 1), 16, 20, 2, False), ((4, 129, 70, 200, 1), 8, 10, 3, True)]
IDS = ["per_lane_A4", "large_actions_A129"]


def _heads(shape, seed):
    model = mr.fresh_net(*shape, seed=seed, gain=GAIN)
    heads = model.heads("cuda:0", backend="broad")
    assert type(heads).__name__ == "HipMlpBroadHeads" and heads.single_launch is None
    return model, heads


@pytest.mark.parametrize("shape,B,sims,K,large", CASES, ids=IDS)
def test_expand_consumes_what_the_broad_heads_wrote(shape, B, sims, K, large):
    """A second engine fed the recorded head outputs builds the same trees and leaves the same stream positions, bit for bit;
    every round's outputs are within the bounds of the restatement on that round's inputs."""
    model, heads = _heads(shape, 31 + int(large))
    rec = _Recording(heads)
    seeds, obs = np.arange(B, dtype=np.uint64) + 7, _obs(B, shape[0], 8)
    _, eng = _search(B, rec, obs, seeds, sims, K)
    assert bool(eng.large_actions) == large and eng.A == shape[1] and len(rec.rounds) == sims
    assert (eng.root_stats()[0].sum(1) == sims).all()
    _, again = _search(B, _Tape(rec), obs, seeds, sims, K)
    _trees_equal(eng, again, B)
    _streams_equal(eng, again, B)
    _rounds_match_the_restatement(f"broad search A{shape[1]}", model, rec)


@pytest.mark.parametrize("shape,B,sims,K,large", CASES, ids=IDS)
def test_graph_equals_eager(shape, B, sims, K, large, recwarn):
    """use_graph=True and use_graph=False give identical trees; no single-launch search is attempted on these heads."""
    mcts_mod = _pkg("mcts")
    _, heads = _heads(shape, 33 + int(large))
    obs = _obs(B, shape[0], 9)
    out = []
    for use_graph in (True, False):
        mc = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=K, use_graph=use_graph)
        mc.seed(np.arange(B, dtype=np.uint64))
        eng = mc.run(obs, heads, train=True)
        assert bool(eng.large_actions) == large and (mc._graph is not None) == use_graph
        v, p, rv, cr = (x.clone() for x in eng.root_stats())
        out.append((v, p, rv, eng.act(1.0)[0].clone()))
        assert int(v.sum()) == B * sims
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert not [w for w in recwarn if "single-launch" in str(w.message)]
