"""Step-wise searches whose recurrent networks are the bf16 broad HIP heads (heads.HipMlpBroadBf16Heads,
Muzero.heads(backend="broad_bf16")): a round is three launches -- select, smz_mlp_recurrent_broad_bf16, expand + backup -- on a
per-lane handle (A = 4) and on a large-action handle (A = 129); the root is FusedMlpHeads.initial, in float32 on the torch GEMMs.

The method is that of tests/test_gpu_broad_heads_search.py (_Recording / _Tape / _search, imported): the recorded head outputs
of every round are replayed as a tape on a second engine, which must build the same trees and leave the same stream positions
bit for bit (expand consumed exactly what the heads wrote, in the rows select named), and every round's head outputs must be
within the bounds of tests/test_gpu_mlp_broad_bf16_heads.py (check_outputs: the float64 rounded restatement, max(contract,
4 x e32r)) on that round's parent rows, actions and branches (select handed the heads the rows they read).  The captured graph
(smz_mlp_recurrent_broad_bf16 inside it) must give the trees of the eager run; "auto" and "broad" hand out what they handed out."""
import numpy as np
import pytest
import torch

import mlp_bf16_reference as br16
import mlp_reference as mr
from search_helpers import _pkg
from test_gpu_broad_heads_search import GAIN, _obs, _Recording, _search, _Tape
from test_gpu_large_actions import _streams_equal, _trees_equal
from test_gpu_mlp_broad_bf16_heads import check_outputs

pytestmark = pytest.mark.gpu

# (shape (obs, A, S, H, L), trees, simulations, K, large-action handle)
CASES = [((4, 4, 70, 200, 1), 16, 20, 2, False), ((4, 129, 70, 200, 1), 8, 10, 3, True)]
IDS = ["per_lane_A4", "large_actions_A129"]


def _heads(shape, seed):
    model = mr.fresh_net(*shape, seed=seed, gain=GAIN)
    heads = model.heads("cuda:0", backend="broad_bf16")
    assert type(heads).__name__ == "HipMlpBroadBf16Heads" and heads.single_launch is None
    return model, heads


@pytest.mark.parametrize("shape,B,sims,K,large", CASES, ids=IDS)
def test_expand_consumes_what_the_bf16_heads_wrote(shape, B, sims, K, large):
    """A second engine fed the recorded head outputs builds the same trees and leaves the same stream positions, bit for bit;
    every round's outputs are within the bounds of the rounded restatement on that round's inputs."""
    model, heads = _heads(shape, 31 + int(large))
    rec = _Recording(heads)
    seeds, obs = np.arange(B, dtype=np.uint64) + 7, _obs(B, shape[0], 8)
    _, eng = _search(B, rec, obs, seeds, sims, K)
    assert bool(eng.large_actions) == large and eng.A == shape[1] and len(rec.rounds) == sims
    assert (eng.root_stats()[0].sum(1) == sims).all()
    _, again = _search(B, _Tape(rec), obs, seeds, sims, K)
    _trees_equal(eng, again, B)
    _streams_equal(eng, again, B)
    r64, r32r = br16.RoundedRestatement(model), br16.RoundedRestatement(model, torch.float32)
    S = rec.S
    for s, r in enumerate(rec.rounds):
        ph, la, br = r["ph"][:, :S], r["la"].long(), r["br"]
        assert int(la.min()) >= 0 and int(la.max()) < rec.A
        check_outputs(f"broad_bf16 search A{shape[1]} round {s} gain {GAIN}", S, GAIN, r["out"], (ph, la, br), r64.recurrent(ph, la, br),
                      r32r.recurrent(ph, la, br))


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


def test_auto_and_broad_hand_out_what_they_handed_out():
    model = mr.fresh_net(*CASES[0][0], seed=35, gain=GAIN)
    assert type(model.heads("cuda:0")).__name__ == "FusedMlpHeads"
    assert type(model.heads("cuda:0", backend="auto")).__name__ == "FusedMlpHeads"
    assert type(model.heads("cuda:0", backend="broad")).__name__ == "HipMlpBroadHeads"
    assert type(model.heads("cuda:0", backend="broad_bf16", hip_root=True)).__name__ == "HipMlpBroadBf16Heads"      # (hip_root: ignored)
