"""The wave-per-tree tree kernels (csrc/smz_large_actions.hip, smz_large_actions_device.hpp) against the oracle
(oracle/smz_oracle.c: numpy's arithmetic restated, 1 .. 1024 actions) on EVERY tree above 128 actions, where numpy's sums start
to split pairwise and where, before this file, only ten reference trees and the kernels themselves were the evidence.

Every comparison is np.array_equal / ==: there is no tolerance anywhere.  A case checks, on every tree: the selection (action,
branch, parent hidden row) of every simulation; the node arrays, the float64 root priors, MinMax, the last path and the stream
position after the search; act at every golden_util.TEMPERATURES (0, 0.2, 0.5, 1), each continuing the stream; then a second,
shorter search on the same handle and trees, which continues the streams.  S = 8, discount 0.97, exploration fraction 0.25; the
device draws its own Dirichlet gammas (no noise override).  The oracle itself is pinned on the CPU to numpy (test_oracle_rng.py)
and to the reference's own searches with up to 1024 actions (test_large_actions.py).

What each shape is there for:

(a) MT19937, alpha 0.3, train=True; 256 trees, 64 where K = A
    A    K    sims
    129  3    20   one child in the third 64-child pass; pairwise split 64 + 65; a ragged last Dirichlet pass
    200  200  12   K > 128: chance picks sum 200 priors pairwise (96 + 104); `choice` draws 200 a round in passes of 64/64/64/8
                   (400 words); expansion blocks wider than 128
    256  2    20   whole passes only
    313  2    20   one root selection draws 626 words, more than MT19937's 624: it regenerates inside a single selection
                   whatever the start position
    1000 5    20   16 passes, the last one ragged
    1024 2    20   the limit; root slot 1023 fills the 10-bit slot field of the path record
    1024 1024 4    K = A at the limit: every expansion block 1024 wide, slots above 255 below the root
(b) Philox handles against the oracle drawing from the same counter stream (Tree.seed_philox), 256 trees: (33, 2) the first
    width without a per-lane kernel to compare with, (100, 5), (129, 3) past the summation block, (1024, 2) the limit
(c) alpha = 1.0 launches k_root_noise_la<true, *> (two words a round, its own advance arithmetic): (64, 2) one whole pass,
    (129, 3), (1024, 2), on both word sources; alpha = 0.03 at (256, 2): low acceptance, many 32-round passes per root
(d) train=False at (129, 3) and (1024, 2): no noise, the float64 priors are root init's
(e) 0, 1, 2, 3 simulations at A = 129: act's `visits <= 1` (policy from the float64 priors through pow) and `visits < 3`
    (child visits from the priors) branches at every temperature
(f) the chain for the opt-in whole-search kernel at A = 129 and 1024: the step-wise search with HipMlpLargeHeads records every
    network output; the oracle replays that tape on its own trees and must select alike and end alike; then
    BatchedMCTS(large_single_launch=True) on the same seeds and observations must equal the oracle too, act outputs included,
    and its last kernel must be a k_search_mlp_large instantiation
"""
import numpy as np
import pytest
import torch

import golden_util as gu
from test_gpu_fullsize_parity import assert_engine_equals_oracle, oracle_replay
from test_gpu_large_actions import _heads_tape, _run

pytestmark = pytest.mark.gpu

S, DISCOUNT, FRAC = 8, 0.97, 0.25


def _smz():
    import stochastic_muzero_amd as smz
    return smz


def _seeds(B, philox):
    if philox:
        return (np.arange(B, dtype=np.uint64) + np.uint64(3)) * np.uint64(0x9E3779B97F4A7C15)       # full 64-bit keys
    return np.arange(B, dtype=np.uint64) * np.uint64(7919) + np.uint64(11)


def _oracle_trees(A, K, hidden, sims, seeds, alpha, philox):
    import orc
    cfg = orc.make_cfg(A, K, hidden, sims, discount=DISCOUNT, alpha=alpha, frac=FRAC)
    trees = []
    for s in seeds:
        t = orc.Tree(cfg)
        if philox:
            t.seed_philox(int(s))
        else:
            t.seed(int(s))
        trees.append(t)
    return trees


def _search(eng, trees, root, steps, train):
    """One search on the engine and on every oracle tree (test_gpu_large_actions._run: the oracle must select alike at every
    simulation); with no simulation only the roots are initialised."""
    if steps:
        return _run(eng, root, steps, train=train, oracle=trees)
    for i, t in enumerate(trees):
        t.root_init(root[1][i], hidden=root[0][i], train=train)
    eng.root_init(torch.from_numpy(root[0]).cuda(), torch.from_numpy(root[1]).cuda(), train=train)
    torch.cuda.synchronize()


def _acts_equal_the_oracle(eng, trees):
    """act at every temperature, one after the other: each draw continues the tree's stream on both sides."""
    for T in gu.TEMPERATURES:
        act, pol, cv, rv = (x.cpu().numpy() for x in eng.act(T))
        for i, t in enumerate(trees):
            oa, opol, ocv, orv = t.act(T)
            assert act[i] == oa, (T, i, act[i], oa)
            assert np.array_equal(pol[i], opol), (T, i, "policy")
            assert np.array_equal(cv[i], ocv), (T, i, "child visits")
            assert rv[i] == orv, (T, i, rv[i], orv)


def _every_tree_equals_the_oracle(A, K, B, sims, philox=False, alpha=0.3, train=True):
    smz = _smz()
    eng = smz.SearchEngine(B, A, S, num_simulations=sims, maxium_action_sample=K, discount=DISCOUNT, root_dirichlet_alpha=alpha,
                           root_exploration_fraction=FRAC, large_actions=True,
                           rng_mode=smz._lib.RNG_PHILOX if philox else smz._lib.RNG_MT19937_NUMPY)
    seeds = _seeds(B, philox)
    eng.seed(seeds)
    trees = _oracle_trees(A, K, S, sims, seeds, alpha, philox)
    root, steps = _heads_tape(B, A, S, sims, seed=A * 1000 + K)
    _search(eng, trees, root, steps, train)
    assert_engine_equals_oracle(eng, trees, sims, prior_rtol=0)
    _acts_equal_the_oracle(eng, trees)
    sims2 = sims // 2
    root2, steps2 = _heads_tape(B, A, S, sims2, seed=A + K)
    _search(eng, trees, root2, steps2, train)
    assert_engine_equals_oracle(eng, trees, sims2, prior_rtol=0)      # (the stream position after the acts is in here too)
    eng.close()


@pytest.mark.parametrize("A,K,sims", [(129, 3, 20), (200, 200, 12), (256, 2, 20), (313, 2, 20), (1000, 5, 20), (1024, 2, 20),
                                      (1024, 1024, 4)])
def test_mt19937_trees_above_128_actions_equal_the_oracle(A, K, sims):
    """(a): the smallest shapes at which each path above 128 actions can go wrong (module docstring)."""
    _every_tree_equals_the_oracle(A, K, 64 if K == A else 256, sims)


@pytest.mark.parametrize("A,K", [(33, 2), (100, 5), (129, 3), (1024, 2)])
def test_philox_trees_above_32_actions_equal_the_oracle(A, K):
    """(b): Philox handles have no per-lane kernel to be compared with above 32 actions; the oracle draws from the same
    counter stream, and the (block, index) position is compared after every search."""
    _every_tree_equals_the_oracle(A, K, 256, 20, philox=True)


@pytest.mark.parametrize("philox", [False, True])
@pytest.mark.parametrize("A,K", [(64, 2), (129, 3), (1024, 2)])
def test_alpha_one_noise_kernel_equals_the_oracle(A, K, philox):
    """(c): root_dirichlet_alpha == 1.0 is its own instantiation of the noise kernel (-log(1 - u) per action, two words each)."""
    _every_tree_equals_the_oracle(A, K, 256, 20, philox=philox, alpha=1.0)


def test_low_acceptance_alpha_equals_the_oracle():
    """(c): alpha = 0.03 at (256, 2): most rounds of the gamma rejection loop fail, so every root takes many 32-round passes."""
    _every_tree_equals_the_oracle(256, 2, 256, 20, alpha=0.03)


@pytest.mark.parametrize("A,K", [(129, 3), (1024, 2)])
def test_searches_without_noise_equal_the_oracle(A, K):
    """(d): train=False."""
    _every_tree_equals_the_oracle(A, K, 256, 20, train=False)


@pytest.mark.parametrize("sims", [0, 1, 2, 3])
def test_few_visits_act_equals_the_oracle(sims):
    """(e): A = 129 with 0 .. 3 simulations, train=True: act takes its policy from the float64 priors up to one visit
    (pow(prior, 1 / T) at T >= 0.3, glibc's pow on both sides) and its child visits from them below three."""
    _every_tree_equals_the_oracle(129, 3, 256, sims)


# ---- (f) the whole-search kernel, through the oracle -----------------------------------------------------------------------
def _stepwise_tape(heads, obs, seeds, sims, K, alpha):
    """BatchedMCTS._search with HipMlpLargeHeads, one launch at a time, every network output of every simulation kept."""
    smz = _smz()
    B = obs.shape[0]
    hidden, policy = heads.initial(obs)
    torch.cuda.synchronize()
    root = hidden.cpu().numpy().copy(), policy.cpu().numpy().copy()
    eng = smz.SearchEngine(B, heads.A, heads.S, num_simulations=sims, maxium_action_sample=K, discount=DISCOUNT,
                           root_dirichlet_alpha=alpha, root_exploration_fraction=FRAC, large_actions=True)
    eng.seed(seeds)
    eng.root_init(hidden, policy, train=True)
    tape = []
    for _ in range(sims):
        eng.select(want_mlp_input=False, want_parent_hidden=True)
        h2, rw, pol, val = heads.recurrent(eng)
        torch.cuda.synchronize()
        tape.append(dict(action=eng.last_action.cpu().numpy().copy(), branch=eng.branch.cpu().numpy().copy(),
                         parent_hidden=eng.parent_hidden.cpu().numpy()[:, :heads.S].copy(), hidden=h2.cpu().numpy().copy(),
                         reward=rw.cpu().numpy().copy(), policy=pol.cpu().numpy().copy(), value=val.cpu().numpy().copy()))
        eng.expand_backup(h2, rw, pol, val)
    torch.cuda.synchronize()
    return eng, root, tape


@pytest.mark.parametrize("A", [129, 1024])
def test_large_single_launch_equals_the_oracle_on_every_tree(A):
    """(f): step-wise search -> tape -> oracle -> k_search_mlp_large, K = 2, 64 trees, 12 simulations."""
    from importlib import import_module
    import mlp_reference as mr
    _smz()
    K, B, sims, alpha = 2, 64, 12, 0.3
    heads = mr.fresh_net(6, A, 16, 64, 1, gain=4).heads("cuda:0", backend="large")
    assert type(heads).__name__ == "HipMlpLargeHeads"
    obs = (torch.rand(B, 6, generator=torch.Generator().manual_seed(A)) - 0.5).cuda().contiguous()
    seeds = _seeds(B, False)
    # (1) + (2) + (3): the step-wise kernels, and the oracle on their tape
    eng, root, tape = _stepwise_tape(heads, obs, seeds, sims, K, alpha)
    trees = _oracle_trees(A, K, heads.S, sims, seeds, alpha, False)
    for i, t in enumerate(trees):
        t.root_init(root[1][i], hidden=root[0][i], train=True)
    oracle_replay(trees, tape)
    assert_engine_equals_oracle(eng, trees, sims, prior_rtol=0)
    eng.close()
    # (4): all rounds in one launch, same seeds and observations
    mc = import_module("stochastic-muzero_amd.mcts").BatchedMCTS(
        B, num_simulations=sims, maxium_action_sample=K, discount=DISCOUNT, root_dirichlet_alpha=alpha,
        root_exploration_fraction=FRAC, use_graph=False, large_single_launch=True)
    mc.seed(seeds)
    single = mc.run(obs, heads, train=True)
    torch.cuda.synchronize()
    assert single.large_actions and single.last_kernel().startswith("k_search_mlp_large"), single.last_kernel()
    assert_engine_equals_oracle(single, trees, sims, prior_rtol=0)
    _acts_equal_the_oracle(single, trees)
    assert_engine_equals_oracle(single, trees, sims, prior_rtol=0)    # the streams after the acts
