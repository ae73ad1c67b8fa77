"""Step-wise searches whose recurrent networks are the large-action HIP heads (heads.HipMlpLargeHeads, Muzero.heads(backend=
"large")): a round is three launches -- select, smz_mlp_recurrent_large, expand + backup -- on a large-action handle.

What stands in for the trees' reference.  oracle/smz_oracle.c knows one player, so:
  * the bit-for-bit replay against orc.Tree runs at A = 128 (K = 3, 20 simulations, 8 trees; the same chain at 129 and 1024
    actions, with the whole-search kernel at its end, is in tests/test_gpu_large_actions_oracle.py);
  * at A = 256, and with two players at A = 64, the recorded head outputs of every round are replayed as a tape on a second
    engine, which must build the same trees bit for bit (expand consumed exactly what the heads wrote, in the rows select
    named), and every round's head outputs must be the float64 restatement's on that round's parent rows, actions and
    branches (select handed the heads the rows they read).  The two-player trees differ from the one-player trees grown from
    the same tape: the signed backup saw the heads' values.
The engine's trees at 33 .. 1000 actions and with two players are held to the reference's own fixtures elsewhere
(tests/test_gpu_large_actions.py, tests/test_gpu_players.py)."""
import numpy as np
import pytest
import torch

import mlp_reference as mr
from search_helpers import _pkg
from test_gpu_large_actions import _streams_equal, _trees_equal
from test_gpu_lstm import _held
from test_gpu_lstm_envelope import _decoded, _hidden_rows
from test_gpu_mlp_envelope import TILE_ATOL

pytestmark = pytest.mark.gpu
GAIN = 4


def _obs(B, n, seed):
    return (torch.rand(B, n, generator=torch.Generator().manual_seed(seed)) - 0.5).cuda().contiguous()


class _Recording:
    """The heads, with every round's inputs and outputs copied to the host."""
    wants_mlp_input, wants_parent_hidden = False, True

    def __init__(self, heads):
        self.heads, self.A, self.S = heads, heads.A, heads.S
        self.root, self.rounds = None, []

    def initial(self, obs):
        h, p = self.heads.initial(obs)
        self.root, self.rounds = (h.cpu().clone(), p.cpu().clone()), []
        return h, p

    def recurrent(self, eng):
        out = self.heads.recurrent(eng)
        torch.cuda.synchronize()
        self.rounds.append(dict(ph=eng.parent_hidden.cpu().clone(), la=eng.last_action.cpu().clone(), br=eng.branch.cpu().clone(),
                                out=[t.cpu().clone() for t in out]))
        return out


class _Tape:
    """Heads that replay a recording."""
    wants_mlp_input, wants_parent_hidden = False, True

    def __init__(self, rec):
        self.A, self.S, self.s = rec.A, rec.S, 0
        self.root = [t.cuda() for t in rec.root]
        self.rounds = [[t.cuda() for t in r["out"]] for r in rec.rounds]

    def initial(self, obs):
        self.s = 0
        return self.root

    def recurrent(self, eng):
        self.s += 1
        return self.rounds[self.s - 1]


def _rounds_match_the_restatement(tag, model, rec):
    """Every round's four outputs against the restatement on that round's inputs, bounds as in test_gpu_mlp_large_heads.py."""
    r64, r32 = mr.Restatement(model), mr.Restatement(model, torch.float32)
    S = rec.S
    for s, r in enumerate(rec.rounds):
        ph, la, br = r["ph"][:, :S], r["la"].long(), r["br"]
        assert int(la.min()) >= 0 and int(la.max()) < rec.A
        out64, out32 = r64.recurrent(ph, la, br), r32.recurrent(ph, la, br)
        bound = {k: max(TILE_ATOL[k], 4 * float((out64[k] - out32[k].double()).abs().max())) for k in ("hidden", "policy")}
        h2, rw, p2, v2 = r["out"]
        keep = _hidden_rows(out64["span"], S)
        assert bool(keep.all())
        _held(f"{tag} round {s} hidden", h2, out64["hidden"], bound["hidden"])
        _held(f"{tag} round {s} policy", p2, out64["policy"], bound["policy"])
        assert (rw[br == 0] == 0).all()
        if bool((br != 0).any()):
            _decoded(f"{tag} round {s} reward", rw, out64, out32, "reward", GAIN, br != 0)
        _decoded(f"{tag} round {s} value", v2, out64, out32, "value", GAIN, torch.ones_like(br, dtype=torch.bool))


def _search(B, heads, obs, seeds, sims, K, **kw):
    mc = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, maxium_action_sample=K, use_graph=False,
                                  **{k: v for k, v in kw.items() if k != "to_play"})
    mc.seed(seeds)
    eng = mc.run(obs, heads, train=True, **({"to_play": kw["to_play"]} if "to_play" in kw else {}))
    torch.cuda.synchronize()
    return mc, eng


@pytest.mark.parametrize("philox", [False, True], ids=["mt19937", "philox"])
def test_graph_equals_eager_at_256_actions(philox, recwarn):
    """BatchedMCTS(128, 20 simulations, K = 2) on a fresh (6,256,16,64,1) net with the large heads: an LA engine, no
    single-launch attempt, and the captured graph (smz_mlp_recurrent_large inside it) equals the eager step-wise run."""
    mcts_mod = _pkg("mcts")
    A, B, sims = 256, 128, 20
    model = mr.fresh_net(6, A, 16, 64, 1, seed=21, gain=GAIN)
    heads = model.heads("cuda:0", backend="large")
    assert type(heads).__name__ == "HipMlpLargeHeads"
    obs = _obs(B, 6, 3)
    out = []
    for use_graph in (True, False):
        mc = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, use_graph=use_graph,
                                  rng_mode="philox" if philox else "mt19937")
        mc.seed(np.arange(B, dtype=np.uint64))
        eng = mc.run(obs, heads, train=True)
        assert eng.large_actions and eng.A == A
        assert (mc._graph is not None) == use_graph
        v, p, rv, cr = (x.clone() for x in eng.root_stats())
        assert p.dtype == torch.float64
        out.append((v, p, rv, eng.act(1.0)[0].clone()))
        assert int(v.sum()) == B * sims
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert not [w for w in recwarn if "single-launch" in str(w.message)]


def test_the_trees_are_the_oracles_on_the_heads_own_outputs():
    """Eager step-wise search, B = 8, A = 128 (the oracle's limit: module docstring), K = 3, 20 simulations: orc.Tree replays
    every round with the four head outputs copied to the host; selections, parent rows, final trees and stream positions match
    bit for bit, and every round's head outputs are the restatement's on that round's inputs."""
    import orc
    from test_gpu_fullsize_parity import assert_engine_equals_oracle
    A, S, B, sims, K = 128, 16, 8, 20, 3
    model = mr.fresh_net(6, A, S, 64, 1, seed=22, gain=GAIN)
    rec = _Recording(model.heads("cuda:0", backend="large"))
    seeds = np.arange(B, dtype=np.uint64) + 11
    _, eng = _search(B, rec, _obs(B, 6, 4), seeds, sims, K)
    assert eng.large_actions and len(rec.rounds) == sims
    cfg = orc.make_cfg(A, K, S, sims)
    trees = []
    h0, p0 = (t.numpy() for t in rec.root)
    for i in range(B):
        t = orc.Tree(cfg)
        t.seed(int(seeds[i]))
        t.root_init(p0[i], hidden=h0[i], train=True)
        for s, r in enumerate(rec.rounds):
            _, _, oa, of, oph = t.select(want_hidden=True)
            assert (oa, of) == (int(r["la"][i]), int(r["br"][i])), f"simulation {s}, tree {i}"
            assert np.array_equal(oph[:S], r["ph"][i].numpy()[:S]), f"simulation {s}, tree {i}: parent hidden row"
            h, rw, p, v = (x.numpy() for x in r["out"])
            t.expand_backup(p[i], v[i], reward=rw[i], hidden=h[i])
        trees.append(t)
    assert_engine_equals_oracle(eng, trees, sims, prior_rtol=0)
    _rounds_match_the_restatement("search A128", model, rec)


@pytest.mark.parametrize("A,players", [(256, 1), (64, 2)], ids=["A256", "A64_two_players"])
def test_expand_consumes_what_the_heads_wrote(A, players):
    """B = 8, K = 3, 20 simulations at A = 256, and with number_of_player = 2 at A = 64 (to_play alternating over the trees):
    a second engine fed the recorded head outputs builds the same trees and leaves the same stream positions, bit for bit;
    every round's outputs are the restatement's on that round's inputs.  The heads are oblivious to players, the signed backup
    is not: the same tape searched with one player gives other root values."""
    S, B, sims, K = 16, 8, 20, 3
    model = mr.fresh_net(6, A, S, 64, 1, seed=23 + players, gain=GAIN)
    rec = _Recording(model.heads("cuda:0", backend="large"))
    seeds, obs = np.arange(B, dtype=np.uint64) + 5, _obs(B, 6, 5)
    kw = dict(number_of_player=2, to_play=np.arange(B, dtype=np.int32) % 2) if players == 2 else {}
    _, eng = _search(B, rec, obs, seeds, sims, K, **kw)
    assert eng.large_actions and len(rec.rounds) == sims and getattr(eng, "n_cycle", 1) == players
    visits = eng.root_stats()[0]
    assert (visits.sum(1) == sims).all()
    _, again = _search(B, _Tape(rec), obs, seeds, sims, K, **kw)
    _trees_equal(eng, again, B)
    _streams_equal(eng, again, B)
    _rounds_match_the_restatement(f"search A{A} players {players}", model, rec)
    if players == 2:
        _, one = _search(B, _Tape(rec), obs, seeds, sims, K)
        assert not torch.equal(one.root_stats()[2], eng.root_stats()[2])


def test_inactive_trees_do_not_disturb_their_neighbours():
    """B = 64 with every odd tree switched off (set_active), 10 simulations at A = 256: the active trees' visits are those of a
    32-tree run of the same seeds and observations, the inactive trees have none.  An inactive row's last_action is whatever
    the buffer held (select returns early for it and the test does not write it): the kernel range-checks it."""
    A, B, sims = 256, 64, 10
    model = mr.fresh_net(6, A, 16, 64, 1, seed=26, gain=GAIN)
    heads = model.heads("cuda:0", backend="large")
    obs, seeds = _obs(B, 6, 6), np.arange(B, dtype=np.uint64) + 3
    mcts_mod = _pkg("mcts")
    mc = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, use_graph=False)
    active = (torch.arange(B) % 2 == 0).to(torch.uint8).cuda()
    mc.set_active(active)
    mc.seed(seeds)
    eng = mc.run(obs, heads, train=True)
    visits = eng.root_stats()[0].cpu()
    torch.cuda.synchronize()
    _, half = _search(B // 2, heads, obs[::2].contiguous(), seeds[::2].copy(), sims, 2)
    assert torch.equal(visits[::2], half.root_stats()[0].cpu()) and (visits[::2].sum(1) == sims).all()
    assert (visits[1::2] == 0).all()


def test_weights_updated_in_place_give_new_heads():
    """One p.add_() on a parameter: the next heads(backend="large") is a new object (weights_version), packed from the new
    weights -- its outputs follow the updated net's restatement and differ from the old heads' outputs."""
    from test_gpu_mlp_large_heads import _case, _compare, _engine_rows
    shape = (6, 256, 16, 64, 1)
    case = _case(shape, 27, GAIN, 28, rows=256)
    model, (h, a, br), _, _ = case
    old = model.heads("cuda:0", backend="large")
    assert model.heads("cuda:0", backend="large") is old
    before = [t.clone() for t in old.recurrent(_engine_rows(h, a, br))]
    with torch.no_grad():
        [m for m in model.prediction_function.policy if isinstance(m, torch.nn.Linear)][-1].bias.add_(torch.linspace(-1, 1, shape[1]))
        next(model.dynamics_function.parameters()).add_(0.01)
    new = model.heads("cuda:0", backend="large")
    assert new is not old and type(new).__name__ == "HipMlpLargeHeads"
    r64, r32 = mr.Restatement(model), mr.Restatement(model, torch.float32)
    h2, _, p2, _ = _compare("large after an in-place update", shape, GAIN, new, (model, (h, a, br), r64.recurrent(h, a, br), r32.recurrent(h, a, br)))
    assert not torch.equal(p2, before[2].cpu()) and not torch.equal(h2, before[0].cpu())
