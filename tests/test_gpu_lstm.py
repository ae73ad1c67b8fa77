"""lstm_model on the GPU: HipLstmHeads (csrc/smz_lstm.hip) and LstmTorchHeads against the reference's own network calls and
searches (tools/gen_golden_lstm.py, tests/golden/lstm/), against each other, and inside the search and self-play loops.

Tolerances are those of the vision family's head test (test_gpu_end_to_end.py): 1e-5 on hidden rows, 1e-6 on policies,
decoded scalars within one stair of the reference's decode.  The values quoted in the docstrings are the measured ones;
with SMZ_TOLERANCE_LOG set to a file name, the largest error of each comparison is appended to that file as a JSON line."""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as gu
from test_records import Buffer, same_game

pytestmark = pytest.mark.gpu
NETS = [("lstmnet_cartpole_L1", "lstm_cartpole_sims50"), ("lstmnet_lunar_L2", "lstm_lunarL2_K2_sims30")]


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _model(name):
    return _pkg("model").Muzero.from_state_dicts(os.path.join(gu.GOLDEN, "lstm", name + ".npz"))


class _FakeEngine:
    pass


def _held(what, got, want, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = float(np.abs(got - want).max())
    log = os.environ.get("SMZ_TOLERANCE_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(dict(what=what, max_abs=err, atol=atol)) + "\n")
    assert err <= atol, (what, err, atol)


def _engine_rows(hidden_in, action, branch, A):
    fe = _FakeEngine()
    h = torch.as_tensor(hidden_in, dtype=torch.float32)
    a = torch.as_tensor(action).long()
    fe.mlp_input = torch.cat([h, torch.nn.functional.one_hot(a, A).float()], 1).cuda().contiguous()
    fe.branch = torch.as_tensor(branch).to(torch.uint8).cuda()
    fe.last_action = a.int().cuda()
    fe.B, fe.S = h.shape[0], h.shape[1]
    return fe


@pytest.mark.parametrize("backend", ["hip", "torch"])
@pytest.mark.parametrize("net,tape", NETS)
def test_lstm_heads_on_gpu_match_the_reference_tape(net, tape, backend):
    """Every network call the reference made in its searches (TapeModel), evaluated as one batch per phase.
    Measured on MI355X (hip / torch, worst of the two nets): root hidden rows 1.2e-7 / 6.0e-8, root policies 6.0e-8 / 3.0e-8,
    hidden rows 4.3e-7 / 3.6e-7, policies 6.0e-8 / 6.0e-8; decoded scalars within one stair of the reference's decode."""
    model = _model(net)
    heads = model.heads("cuda:0", backend=backend)
    assert type(heads).__name__ == {"hip": "HipLstmHeads", "torch": "LstmTorchHeads"}[backend]
    cfg, data = gu.load("lstm/" + tape)
    ncase, sims = data["tape_branch"].shape
    A = model.action_dimension
    hid, pol = heads.initial(torch.from_numpy(data["obs"]).cuda().contiguous())
    torch.cuda.synchronize()
    _held(f"{net} {backend} root hidden", hid.cpu(), data["root_hidden"], 1e-5)
    _held(f"{net} {backend} root policy", pol.cpu(), data["root_policy"], 1e-6)
    fe = _engine_rows(data["tape_hidden_in"].reshape(ncase * sims, -1), data["tape_action"].reshape(-1),
                      data["tape_branch"].reshape(-1), A)
    h2, rw, p2, v2 = heads.recurrent(fe)
    torch.cuda.synchronize()
    _held(f"{net} {backend} hidden", h2.cpu(), data["tape_hidden_out"].reshape(ncase * sims, -1), 1e-5)
    _held(f"{net} {backend} policy", p2.cpu(), data["tape_policy"].reshape(ncase * sims, -1), 1e-6)
    gu.assert_decoded_like_the_reference(rw.cpu().numpy(), data["tape_reward"], "reward")
    gu.assert_decoded_like_the_reference(v2.cpu().numpy(), data["tape_value"], "value")


@pytest.mark.parametrize("net", [n for n, _ in NETS])
def test_hip_lstm_heads_agree_with_the_torch_heads_on_a_large_batch(net):
    """4096 random rows of mixed branches, and 4096 observations: the HIP kernels (folded input layer, forget gate dropped)
    vs LstmTorchHeads (the modules' own parameters, unfolded).  Measured: root hidden 2.4e-7, root policy 6.0e-8, hidden
    4.2e-7, policy 6.0e-8; decoded scalars within one stair."""
    model = _model(net)
    hip, ref = model.heads("cuda:0", backend="hip"), model.heads("cuda:0", backend="torch")
    A, S, B = model.action_dimension, model.state_dimension, 4096
    g = torch.Generator().manual_seed(5)
    obs = (torch.rand(B, model.observation_dimension, generator=g) - 0.5).cuda()
    (h_a, p_a), (h_b, p_b) = hip.initial(obs), ref.initial(obs)
    torch.cuda.synchronize()
    _held(f"{net} hip vs torch root hidden", h_a.cpu(), h_b.cpu(), 1e-5)
    _held(f"{net} hip vs torch root policy", p_a.cpu(), p_b.cpu(), 1e-6)
    fe = _engine_rows(torch.rand(B, S, generator=g), torch.randint(0, A, (B,), generator=g),
                      torch.randint(0, 2, (B,), generator=g), A)
    assert 0.4 < float(fe.branch.float().mean()) < 0.6
    out_a = [t.clone() for t in hip.recurrent(fe)]
    out_b = [t.clone() for t in ref.recurrent(fe)]
    torch.cuda.synchronize()
    _held(f"{net} hip vs torch hidden", out_a[0].cpu(), out_b[0].cpu(), 1e-5)
    _held(f"{net} hip vs torch policy", out_a[2].cpu(), out_b[2].cpu(), 1e-6)
    assert (out_a[1].cpu()[fe.branch.cpu() == 0] == 0).all()
    gu.assert_decoded_like_the_reference(out_a[1].cpu().numpy(), out_b[1].cpu().numpy(), "reward")
    gu.assert_decoded_like_the_reference(out_a[3].cpu().numpy(), out_b[3].cpu().numpy(), "value")


@pytest.mark.parametrize("backend", ["hip", "torch"])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("net,tape", NETS)
def test_lstm_search_reproduces_the_reference_visit_counts(net, tape, use_graph, backend):
    """Whole searches (observation -> representation -> simulations -> root statistics): tree i under numpy seed i,
    against the reference's own run.  Visit counts equal; root priors within 1e-7 (measured 6.0e-8: one float32 rounding
    of the policy); root values within 1e-5 (measured 4.9e-6 on the L 1 net, 0 on the L 2 net, both backends).
    The fresh L 1 net's outputs are nearly constant, so the min-max-normalised values of one tree hinge on the last bits of
    the heads: with tanh as 1 - 2 / (e^2x + 1) for small arguments (13 ulp on the logits) the HIP searches of that net did
    not give these counts (a CPU emulation of that arithmetic inside the reference's search flips tree 10)."""
    mcts_mod = _pkg("mcts")
    model = _model(net)
    cfg, data = gu.load("lstm/" + tape)
    B = data["seed"].shape[0]
    obs = torch.from_numpy(data["obs"]).cuda().contiguous()
    m = mcts_mod.BatchedMCTS(B, num_simulations=int(cfg["num_simulations"]),
                             maxium_action_sample=int(cfg["maxium_action_sample"]), discount=float(cfg["discount"]),
                             root_dirichlet_alpha=float(cfg["root_dirichlet_alpha"]),
                             root_exploration_fraction=float(cfg["root_exploration_fraction"]), use_graph=use_graph)
    heads = model.heads("cuda:0", backend=backend)
    for _ in range(2 if use_graph else 1):       # the second pass replays the captured graph
        m.seed(data["seed"].astype(np.uint64))
        eng = m.run(obs, heads, train=True)
    visits, priors, root_value, _ = eng.root_stats()
    torch.cuda.synchronize()
    assert m._single is None and (m._graph is not None) == use_graph
    differ = np.flatnonzero((visits.cpu().numpy() != data["root_visits"]).any(1))
    assert differ.size == 0, (differ, visits.cpu().numpy()[differ], data["root_visits"][differ])
    _held(f"{net} search {backend} graph={use_graph} root priors", priors.cpu().numpy(), data["root_priors"], 1e-7)
    _held(f"{net} search {backend} graph={use_graph} root value", root_value.cpu().numpy(), data["root_value"], 1e-5)


def test_default_heads_are_the_hip_kernels():
    heads_mod = _pkg("heads")
    model = _model("lstmnet_cartpole_L1")
    assert isinstance(model.heads("cuda:0"), heads_mod.HipLstmHeads)
    assert isinstance(model.heads("cuda:0", backend="torch"), heads_mod.LstmTorchHeads)


def test_self_play_with_an_lstm_model_is_the_same_with_and_without_graph_capture():
    """A short self_play_iteration (64 CartPole envs, 20 steps, game after game) with the lstm net: the games handed to
    the buffer are identical whether the step-wise search is captured in a graph or launched kernel by kernel."""
    envs_mod, sp, mcts_mod = _pkg("envs"), _pkg("selfplay"), _pkg("mcts")
    model = _model("lstmnet_cartpole_L1")
    res = []
    for use_graph in (False, True):
        env = envs_mod.CartPoleVec(64, "cuda:0", seed=1, on_end="reset", limit=7)
        m = mcts_mod.BatchedMCTS(64, num_simulations=8, discount=0.999, root_exploration_fraction=0.1, use_graph=use_graph)
        m.seed(np.arange(64, dtype=np.uint64))
        buf = Buffer(4, 5)
        games, mean = sp.self_play_iteration(env, model, m, 1.0, 20, replay_buffer=buf)
        assert (m._graph is not None) == use_graph
        res.append((games, mean, buf))
    (ga, ma, ba), (gb, mb, bb) = res
    assert len(ga) == len(gb) > 64 and ma == mb
    for a, b in zip(ga, gb):
        same_game(a, b, 4)
    assert ba.total == bb.total and ba.prio_game == bb.prio_game
