"""smz_search_mlp_wide: the whole search of every tree in one launch for the wide mlp_model shapes
(csrc/smz_mlp_wide_search.hip), opt-in through BatchedMCTS(wide_single_launch=True), against the step-wise kernels with the same
HipMlpTileHeads.  The network phase of the kernel is the tile body of k_mlp_recurrent_wide (csrc/smz_mlp_wide_device.hpp),
compiled with the same flags, a leaf's result does not depend on its tile mates, and the tree phases are the step-wise kernels'
device functions drawing from the same streams: every comparison between the two paths is np.array_equal.  Against the
reference's recorded searches the bound is the step-wise path's (test_gpu_end_to_end.py): the same visit counts on every case."""
import os
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import mlp_reference as mr
from search_helpers import _lib, _pkg, _rng, _same_dumps, _same_states, _snapshot
from test_records import Buffer, same_game

pytestmark = pytest.mark.gpu

# trees per wavefront = ceil(B / 1024): one workgroup of four wavefronts on each of 256 CUs before a wave takes a second tree
# (the kernel is register-bound to one workgroup per CU)
TPW2 = 1 * 256 * 4 + 1                    # the smallest batch whose wavefronts own two trees

# (obs, A, S, H, L): the smallest shape the LDS layout refuses (2 S > 64); H > 64 with hidden layers and four actions
FRESH = {"s33": (4, 2, 33, 64, 0), "h72": (4, 4, 16, 72, 2)}
FIXTURES = {"ckpt450": ("weights_ckpt450.npz", "ckpt450_sims11"), "cfg434": ("weights_cfg434shape.npz", "cfg434shape_sims11")}
NETS = ["s33", "h72", "ckpt450", "cfg434"]


_MODELS = {}


def _net(name):
    """(model, HipMlpTileHeads), built once per net and shared."""
    if name not in _MODELS:
        if name in FRESH:
            model = mr.fresh_net(*FRESH[name], seed=5, gain=3)
        else:
            model = _pkg("model").Muzero.from_arrays(os.path.join(gu.GOLDEN, FIXTURES[name][0]))
        heads = model.heads("cuda:0")
        assert type(heads).__name__ == "HipMlpTileHeads"
        _MODELS[name] = (model, heads)
    return _MODELS[name]


def _obs(B, seed=3):
    return (torch.rand(B, 4, generator=torch.Generator().manual_seed(seed)) - 0.5).mul(0.1).cuda().contiguous()


def _search_pair(heads, B, sims, rng, K=2):
    """Two consecutive searches per engine (the second with the action selection in the launch's tail), single launch and
    step-wise: root statistics, act outputs, three dumped trees and their stream positions."""
    mcts_mod = _pkg("mcts")
    obs = _obs(B)
    res = []
    for single in (True, False):
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=K, discount=0.997, root_exploration_fraction=0.25,
                                 use_graph=False, wide_single_launch=single, rng_mode=_rng(rng))
        m.seed(np.arange(B, dtype=np.uint64) + 9)
        for rep in range(2):
            e = m.run(obs, heads, train=True, act_temperature=(1.0 if single and rep == 1 else None))
        assert m._single is (True if single else None)
        if single:
            assert e.last_kernel().startswith("k_search_mlp_wide<"), e.last_kernel()
        else:
            assert not e.last_kernel().startswith("k_search_mlp_wide<"), e.last_kernel()
        action, policy, cv, rv2 = (t.clone() for t in e.act(1.0))
        visits, priors, rv, cr = e.root_stats()
        torch.cuda.synchronize()
        out = [t.cpu().numpy().copy() for t in (visits, priors, rv, cr, action, policy, cv, rv2)]
        res.append((out, _snapshot(e, rng, sorted({0, B // 2, B - 1}))))
    return res


# (B, sims, forced trees per wavefront or None): a single tree; a partly filled workgroup; 64 trees with 0, 1 and 8 simulations;
# 68 trees as the geometry puts them (one per wavefront) and with five per wavefront -- 20 leaves in a workgroup, so more than 16
# of one branch in the first rounds (two tiles of it), and a last workgroup with a partly filled and two idle wavefronts; two
# trees per wavefront with an odd remainder (the last wavefront owns one tree) and with idle wavefronts in the last workgroup
SHAPES = [(1, 8, None), (5, 8, None), (64, 0, None), (64, 1, None), (64, 8, None), (68, 8, None), (68, 8, 5),
          (TPW2 + 2, 8, None), (TPW2 + 3, 8, None)]


@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("B,sims,tpw", SHAPES)
@pytest.mark.parametrize("net", NETS)
def test_wide_single_launch_search_equals_stepwise_search(net, B, sims, tpw, rng, monkeypatch):
    _, heads = _net(net)
    if tpw is not None:
        monkeypatch.setenv("SMZ_WIDE_SEARCH_TPW", str(tpw))
    # (four actions: every action sampled, the run-time child count of the tree code)
    one, step = _search_pair(heads, B, sims, rng, K=4 if heads.A == 4 else 2)
    for a, b in zip(one[0], step[0]):
        assert np.array_equal(a, b)
    if sims > 0:
        assert (one[0][0].sum(1) == sims).all()
    _same_dumps(one[1][0], step[1][0])
    _same_states(one[1][1], step[1][1], rng)


@pytest.mark.parametrize("net", ["ckpt450", "cfg434"])
def test_wide_single_launch_search_reproduces_the_reference_visit_counts(net):
    """The reference's recorded searches (case i under the fixture's seed i, the fixture's hyper-parameters): the same visit
    counts on every case -- what test_gpu_end_to_end.py holds the step-wise path to."""
    mcts_mod = _pkg("mcts")
    _, heads = _net(net)
    cfg, data = gu.load(FIXTURES[net][1])
    ncase = data["tape_branch"].shape[0]
    m = mcts_mod.BatchedMCTS(ncase, num_simulations=int(cfg["num_simulations"]), maxium_action_sample=2,
                             discount=float(cfg["discount"]), root_dirichlet_alpha=float(cfg["root_dirichlet_alpha"]),
                             root_exploration_fraction=float(cfg["root_exploration_fraction"]), use_graph=False,
                             wide_single_launch=True)
    m.seed(np.asarray(data["seed"], np.uint64))
    e = m.run(torch.from_numpy(data["obs"]).cuda(), heads, train=True)
    visits = e.root_stats()[0]
    torch.cuda.synchronize()
    assert m._single is True and e.last_kernel().startswith("k_search_mlp_wide<")
    assert np.array_equal(visits.cpu().numpy(), data["root_visits"])


@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_masked_trees_are_left_alone(rng):
    """64 trees, every third switched off (smz_set_active) after one full search, and trees 12..15 -- one whole workgroup --
    as well: the active trees equal the step-wise search under the same mask; the dumped arrays and stream positions of the
    masked trees are what they were before the launch."""
    mcts_mod = _pkg("mcts")
    _, heads = _net("cfg434")
    B, sims = 64, 8
    obs = _obs(B)
    active = torch.ones(B, dtype=torch.uint8)
    active[::3] = 0
    active[12:16] = 0                       # (one tree per wavefront at this batch: workgroup 3 owns trees 12..15)
    off, on = [int(i) for i in np.flatnonzero(active.numpy() == 0)], [int(i) for i in np.flatnonzero(active.numpy())]
    active = active.cuda()
    res = []
    for single in (True, False):
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, discount=0.997, use_graph=False, wide_single_launch=single,
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
    _, heads = _net("s33")
    B, sims = 16, 4
    obs = _obs(B)
    # a two-player search with the flag on runs step-wise, without a word
    m = mcts_mod.BatchedMCTS(B, num_simulations=sims, number_of_player=2, use_graph=False, wide_single_launch=True)
    m.seed(np.arange(B, dtype=np.uint64))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        e = m.run(obs, heads, train=True)
        torch.cuda.synchronize()
    assert not [w for w in seen if "single-launch" in str(w.message)]
    assert m._single is None and not e.last_kernel().startswith("k_search_mlp_wide<")
    hidden, policy = heads.initial(obs)
    # ... and the entry point itself refuses such an engine
    with pytest.raises(lib.SmzError) as err:
        e.search_mlp_wide(heads.wide_desc, heads.packed, hidden, policy)
    assert err.value.code == lib.SMZ_ERR_INVALID
    # a large-action engine
    big = eng_mod.SearchEngine(B, heads.A, heads.S, num_simulations=sims, large_actions=True)
    with pytest.raises(lib.SmzError) as err:
        big.search_mlp_wide(heads.wide_desc, heads.packed, hidden, policy)
    assert err.value.code == lib.SMZ_ERR_TOO_LARGE
    big.close()
    plain = eng_mod.SearchEngine(B, heads.A, heads.S, num_simulations=sims)
    # three actions: no instantiation
    three = mr.fresh_net(4, 3, 33, 64, 0, seed=2).heads("cuda:0")
    assert type(three).__name__ == "HipMlpTileHeads"
    eng3 = eng_mod.SearchEngine(B, 3, three.S, num_simulations=sims)
    h3, p3 = three.initial(obs)
    with pytest.raises(lib.SmzError) as err:
        eng3.search_mlp_wide(three.wide_desc, three.packed, h3, p3)
    assert err.value.code == lib.SMZ_ERR_TOO_LARGE
    eng3.close()
    # a descriptor of the LDS layout (OP 64)
    small = mr.fresh_net(4, 2, 16, 32, 0, seed=2).heads("cuda:0", backend="hip")
    assert small.desc.OP == 64
    with pytest.raises(lib.SmzError) as err:
        plain.search_mlp_wide(small.desc, small.weights, hidden, policy)
    assert err.value.code == lib.SMZ_ERR_INVALID
    # a descriptor whose action count is not the engine's
    four = _net("h72")[1]
    other = eng_mod.SearchEngine(B, four.A, heads.S, num_simulations=sims)
    with pytest.raises(lib.SmzError) as err:
        other.search_mlp_wide(heads.wide_desc, heads.packed, hidden, torch.full((B, four.A), 0.25, device="cuda"))
    assert err.value.code == lib.SMZ_ERR_INVALID
    other.close()
    plain.close()


def test_an_action_count_without_an_instantiation_warns_once_and_searches_stepwise():
    """Three actions (bucket 4, not the bucket's own count): smz_search_mlp_wide answers SMZ_ERR_TOO_LARGE; BatchedMCTS says so
    once over two runs and gives the step-wise result."""
    mcts_mod = _pkg("mcts")
    heads = mr.fresh_net(4, 3, 33, 64, 0, seed=3, gain=3).heads("cuda:0")
    assert type(heads).__name__ == "HipMlpTileHeads"
    B, sims = 16, 6
    obs = _obs(B)
    res = []
    for single in (True, False):
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, use_graph=False, wide_single_launch=single)
        m.seed(np.arange(B, dtype=np.uint64))
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for _ in range(2):
                e = m.run(obs, heads, train=True)
        assert m._single is (False if single else None)
        assert len([w for w in seen if "single-launch wide mlp search is outside its limits" in str(w.message)]) == (1 if single else 0)
        visits, priors, rv, cr = e.root_stats()
        torch.cuda.synchronize()
        res.append([t.cpu().numpy().copy() for t in (visits, priors, rv, cr)])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_self_play_with_the_single_launch_gives_the_same_games():
    """self_play_iteration over 64 CartPole envs (8 simulations, 20 steps, episodes cut at 7 steps and reset) with the
    config-434-shaped net: the games handed to the buffer are the same with the flag on and off."""
    envs_mod, sp, mcts_mod = _pkg("envs"), _pkg("selfplay"), _pkg("mcts")
    model, _ = _net("cfg434")
    res = []
    for single in (True, False):
        env = envs_mod.CartPoleVec(64, "cuda:0", seed=1, on_end="reset", limit=7)
        m = mcts_mod.BatchedMCTS(64, num_simulations=8, discount=0.999, root_exploration_fraction=0.1, use_graph=False,
                                 wide_single_launch=single)
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
