"""smz_search_lstm: the whole lstm_model search of every tree in one launch (csrc/smz_lstm_search.hip), opt-in through
BatchedMCTS(lstm_single_launch=True), against the step-wise kernels with HipLstmHeads.  The network phase of the kernel is the
row body of k_lstm_recurrent (csrc/smz_lstm_device.hpp), compiled with the same flags, and the tree phases are the step-wise
kernels' device functions drawing from the same streams: every comparison between the two paths is np.array_equal.  Against
the reference's taped searches the bounds are the step-wise path's (test_gpu_lstm.py)."""
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import lstm_reference as lr
from search_helpers import _lib, _rng, _same_dumps, _same_states, _snapshot
from test_gpu_lstm import NETS, _held, _model, _pkg
from test_records import Buffer, same_game

pytestmark = pytest.mark.gpu

# trees per wavefront = ceil(B / 2048) (two workgroups of four wavefronts on each of 256 CUs before a wave takes a second tree)
TPW2 = 2 * 256 * 4 + 1                    # the smallest batch whose wavefronts own two trees


def _obs(model, B, seed=3):
    return (torch.rand(B, model.observation_dimension, generator=torch.Generator().manual_seed(seed)) - 0.5).mul(0.1).cuda().contiguous()


def _search_pair(model, heads, B, sims, rng, active=None):
    """Two consecutive searches per engine (the second with the action selection in the launch's tail), single launch and
    step-wise: root statistics, act outputs, three dumped trees, two stream positions."""
    mcts_mod = _pkg("mcts")
    obs = _obs(model, B)
    res = []
    for single in (True, False):
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, discount=0.997, root_exploration_fraction=0.25,
                                 use_graph=False, lstm_single_launch=single, rng_mode=_rng(rng))
        if active is not None:
            m.set_active(active)
        m.seed(np.arange(B, dtype=np.uint64) + 9)
        for rep in range(2):
            e = m.run(obs, heads, train=True, act_temperature=(1.0 if single and rep == 1 else None))
        assert m._single is (True if single else None)
        if single:
            assert e.last_kernel().startswith("k_search_lstm<"), e.last_kernel()
        action, policy, cv, rv2 = (t.clone() for t in e.act(1.0))
        visits, priors, rv, cr = e.root_stats()
        torch.cuda.synchronize()
        out = [t.cpu().numpy().copy() for t in (visits, priors, rv, cr, action, policy, cv, rv2)]
        res.append((out, _snapshot(e, rng, sorted({0, B // 2, B - 1})), _snapshot(e, rng, sorted({0, B - 1}))[1]))
    return res


# B = 1; 5 (a partly filled second workgroup); 64 with 0, 1, 8 and the fixtures' own simulation counts; two trees per wavefront with
# an odd remainder (2048 + 3: the last wavefront owns one tree) and the smallest such batch plus 3 (idle wavefronts in the last
# workgroup)
SHAPES = [(1, 8), (5, 8), (64, 0), (64, 1), (64, 8), (64, None), (TPW2 + 2, 8), (TPW2 + 3, 8)]


@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("B,sims", SHAPES)
@pytest.mark.parametrize("net,tape", NETS)
def test_lstm_single_launch_search_equals_stepwise_search(net, tape, B, sims, rng):
    model = _model(net)
    heads = model.heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipLstmHeads"
    if sims is None:
        sims = int(gu.load("lstm/" + tape)[0]["num_simulations"])
    one, step = _search_pair(model, heads, B, sims, rng)
    for a, b in zip(one[0], step[0]):
        assert np.array_equal(a, b)
    if sims > 0:
        assert (one[0][0].sum(1) == sims).all()
    _same_dumps(one[1][0], step[1][0])
    _same_states(one[1][1], step[1][1], rng)


@pytest.mark.parametrize("net,tape", NETS)
def test_lstm_single_launch_search_reproduces_the_reference_visit_counts(net, tape):
    """The taped searches of the reference, tree i under numpy seed i: visit counts equal, root priors within 1e-7 and root
    values within 1e-5 -- what test_gpu_lstm.py holds the step-wise path to."""
    mcts_mod = _pkg("mcts")
    model = _model(net)
    cfg, data = gu.load("lstm/" + tape)
    B = data["seed"].shape[0]
    obs = torch.from_numpy(data["obs"]).cuda().contiguous()
    m = mcts_mod.BatchedMCTS(B, num_simulations=int(cfg["num_simulations"]),
                             maxium_action_sample=int(cfg["maxium_action_sample"]), discount=float(cfg["discount"]),
                             root_dirichlet_alpha=float(cfg["root_dirichlet_alpha"]),
                             root_exploration_fraction=float(cfg["root_exploration_fraction"]), use_graph=False,
                             lstm_single_launch=True)
    m.seed(data["seed"].astype(np.uint64))
    eng = m.run(obs, model.heads("cuda:0", backend="hip"), train=True)
    visits, priors, root_value, _ = eng.root_stats()
    torch.cuda.synchronize()
    assert m._single is True and eng.last_kernel().startswith("k_search_lstm<")
    differ = np.flatnonzero((visits.cpu().numpy() != data["root_visits"]).any(1))
    assert differ.size == 0, (differ, visits.cpu().numpy()[differ], data["root_visits"][differ])
    _held(f"{net} single-launch search root priors", priors.cpu().numpy(), data["root_priors"], 1e-7)
    _held(f"{net} single-launch search root value", root_value.cpu().numpy(), data["root_value"], 1e-5)


@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_masked_trees_are_left_alone(rng):
    """64 trees, every third switched off (smz_set_active) after one full search: the active trees equal the step-wise search
    under the same mask; the dumped arrays and stream positions of the masked trees are what they were before the launch."""
    mcts_mod = _pkg("mcts")
    model = _model("lstmnet_cartpole_L1")
    heads = model.heads("cuda:0", backend="hip")
    B, sims = 64, 8
    obs = _obs(model, B)
    active = torch.ones(B, dtype=torch.uint8)
    active[::3] = 0
    off, on = [int(i) for i in np.flatnonzero(active.numpy() == 0)], [int(i) for i in np.flatnonzero(active.numpy())]
    active = active.cuda()
    res = []
    for single in (True, False):
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, discount=0.997, use_graph=False, lstm_single_launch=single,
                                 rng_mode=_rng(rng))
        m.seed(np.arange(B, dtype=np.uint64) + 4)
        e = m.run(obs, heads, train=True)
        torch.cuda.synchronize()
        before = _snapshot(e, rng, off)
        m.set_active(active)
        e = m.run(obs + 0.01, heads, train=True)
        assert m._single is (True if single else None)
        visits, priors, rv, cr = e.root_stats()
        torch.cuda.synchronize()
        after = _snapshot(e, rng, off)
        _same_dumps(before[0], after[0])
        _same_states(before[1], after[1], rng)
        res.append(([t.cpu().numpy()[on].copy() for t in (visits, priors, rv, cr)], _snapshot(e, rng, on)))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    _same_dumps(res[0][1][0], res[1][1][0])
    _same_states(res[0][1][1], res[1][1][1], rng)


def test_refusals_and_fallback():
    lib = _lib()
    mcts_mod, eng_mod = _pkg("mcts"), _pkg("engine")
    model = _model("lstmnet_cartpole_L1")
    heads = model.heads("cuda:0", backend="hip")
    B, sims = 16, 4
    obs = _obs(model, B)
    # a two-player search with the flag on runs step-wise
    m = mcts_mod.BatchedMCTS(B, num_simulations=sims, number_of_player=2, use_graph=False, lstm_single_launch=True)
    m.seed(np.arange(B, dtype=np.uint64))
    e = m.run(obs, heads, train=True)
    torch.cuda.synchronize()
    assert m._single is None and not e.last_kernel().startswith("k_search_lstm<")
    hidden, policy = heads.initial(obs)
    # ... and the entry point itself refuses such an engine
    with pytest.raises(lib.SmzError) as err:
        e.search_lstm(heads.desc, heads.weights, hidden, policy)
    assert err.value.code == lib.SMZ_ERR_INVALID
    # a large-action engine
    big = eng_mod.SearchEngine(B, heads.A, heads.S, num_simulations=sims, large_actions=True)
    with pytest.raises(lib.SmzError) as err:
        big.search_lstm(heads.desc, heads.weights, hidden, policy)
    assert err.value.code == lib.SMZ_ERR_TOO_LARGE
    big.close()
    # a descriptor whose action count is not the engine's
    other = _model("lstmnet_lunar_L2").heads("cuda:0", backend="hip")
    plain = eng_mod.SearchEngine(B, other.A, heads.S, num_simulations=sims)
    with pytest.raises(lib.SmzError) as err:
        plain.search_lstm(heads.desc, heads.weights, hidden, torch.full((B, other.A), 0.25, device="cuda"))
    assert err.value.code == lib.SMZ_ERR_INVALID
    plain.close()


def test_an_action_count_without_an_instantiation_warns_once_and_searches_stepwise():
    """Three actions (bucket 4, not the bucket's own count): smz_search_lstm answers SMZ_ERR_TOO_LARGE; BatchedMCTS says so once
    and gives the step-wise result."""
    mcts_mod = _pkg("mcts")
    model = lr.fresh_net(4, 3, 16, 1, seed=3, gain=2)
    heads = model.heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipLstmHeads"
    B, sims = 16, 6
    obs = _obs(model, B)
    res = []
    for single in (True, False):
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, use_graph=False, lstm_single_launch=single)
        m.seed(np.arange(B, dtype=np.uint64))
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for _ in range(2):
                e = m.run(obs, heads, train=True)
        assert m._single is (False if single else None)
        assert len([w for w in seen if "single-launch lstm search" in str(w.message)]) == (1 if single else 0)
        visits, priors, rv, cr = e.root_stats()
        torch.cuda.synchronize()
        res.append([t.cpu().numpy().copy() for t in (visits, priors, rv, cr)])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_self_play_with_the_single_launch_gives_the_same_games():
    """The loop of test_gpu_lstm.py's self-play test (64 CartPole envs, 8 simulations, 20 steps): the games handed to the buffer
    are the same with the flag on and off."""
    envs_mod, sp, mcts_mod = _pkg("envs"), _pkg("selfplay"), _pkg("mcts")
    model = _model("lstmnet_cartpole_L1")
    res = []
    for single in (True, False):
        env = envs_mod.CartPoleVec(64, "cuda:0", seed=1, on_end="reset", limit=7)
        m = mcts_mod.BatchedMCTS(64, num_simulations=8, discount=0.999, root_exploration_fraction=0.1, use_graph=False,
                                 lstm_single_launch=single)
        m.seed(np.arange(64, dtype=np.uint64))
        buf = Buffer(4, 5)
        games, mean = sp.self_play_iteration(env, model, m, 1.0, 20, replay_buffer=buf)
        assert m._single is (True if single else None)
        res.append((games, mean, buf))
    (ga, ma, ba), (gb, mb, bb) = res
    assert len(ga) == len(gb) > 64 and ma == mb
    for a, b in zip(ga, gb):
        same_game(a, b, 4)
    assert ba.total == bb.total and ba.prio_game == bb.prio_game
