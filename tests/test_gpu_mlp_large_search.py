"""smz_search_mlp_large: all rounds of a large-action search (33 .. 1024 actions, HipMlpLargeHeads) in one launch
(csrc/smz_mlp_large_search.hip), opt-in through BatchedMCTS(large_single_launch=True), against the step-wise kernels with the same
heads, seeds and observations.  Both paths run the same tree device functions and the same tile body (large_tile<4>), so trees,
root statistics and stream positions are compared bit for bit.  Every single-launch run asserts that the engine's last kernel is
a k_search_mlp_large instantiation: a silent fall-back to the step-wise kernels cannot pass.

Nets: mlp_reference.fresh_net(6, A, 16, 64, 1, gain=4).  Shapes: the smallest at which the kernel can go wrong -- fewer actions
than lanes, one / two / eight policy panels with a ragged last one, T = 3 trees per workgroup (A > 768), ragged last workgroups,
more workgroups than the chip has CUs, 0 and 1 rounds.  The launcher gives a workgroup ceil(B / 256) trees, which is one at these
batch sizes; the `geometry` fixture also runs every comparison with SMZ_LARGE_SEARCH_T=4, "as many as fit" (4, or 3 above 768
actions), the geometry the ragged workgroups, the switched-off workgroup and T = 3 belong to."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import mlp_reference as mr
from search_helpers import _pkg
from test_gpu_large_actions import _streams_equal, _trees_equal

pytestmark = pytest.mark.gpu
GAIN = 4
KERNEL = "k_search_mlp_large"


@pytest.fixture(params=["most_that_fit", "one_workgroup_per_cu"])
def geometry(request, monkeypatch):
    """Trees per workgroup: SMZ_LARGE_SEARCH_T=4 (the most that fit, at most 4), or the launcher's own choice."""
    if request.param == "most_that_fit":
        monkeypatch.setenv("SMZ_LARGE_SEARCH_T", "4")
    else:
        monkeypatch.delenv("SMZ_LARGE_SEARCH_T", raising=False)
    return request.param


@functools.lru_cache(maxsize=None)
def _net(A, backend="large"):
    model = mr.fresh_net(6, A, 16, 64, 1, seed=40 + A % 7, gain=GAIN)
    heads = model.heads("cuda:0", backend=backend)
    if backend == "large":
        assert type(heads).__name__ == "HipMlpLargeHeads"
    return model, heads


def _obs(B, seed):
    return (torch.rand(B, 6, generator=torch.Generator().manual_seed(seed)) - 0.5).cuda().contiguous()


def _run(mc, obs, heads, single, train=True, act_temperature=None):
    """One search; returns the engine.  No "single-launch" warning on either path; the single launch names its kernel."""
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        eng = mc.run(obs, heads, train=train, act_temperature=act_temperature)
        torch.cuda.synchronize()
    assert not [w for w in seen if "single-launch" in str(w.message)], [str(w.message) for w in seen]
    assert eng.large_actions
    if single:
        assert eng.last_kernel().startswith(KERNEL), eng.last_kernel()
    else:
        assert not eng.last_kernel().startswith(KERNEL), eng.last_kernel()
    return eng


def _pair(A, K, B, sims, rng, train=True, active=None, backend="large", **kw):
    """The same seeds and observations on two fresh BatchedMCTS objects: step-wise, then large_single_launch=True."""
    _, heads = _net(A, backend)
    obs, seeds = _obs(B, 100 + A + B), np.arange(B, dtype=np.uint64) + 7
    out = []
    for single in (False, True):
        mc = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, maxium_action_sample=K, use_graph=False, rng_mode=rng,
                                      large_single_launch=single, **kw)
        if active is not None:
            mc.set_active(active)
        mc.seed(seeds)
        out.append((mc, _run(mc, obs, heads, single and backend == "large" and kw.get("number_of_player", 1) == 1, train=train)))
    return out


def _equal(a, b, B, trees=None):
    """Trees (all, or the listed ones), all four root statistics and the stream positions."""
    if trees is None:
        _trees_equal(a, b, B)
        _streams_equal(a, b, B)
    else:
        for i in trees:
            da, db = a.dump_tree(i), b.dump_tree(i)
            assert da["n_nodes"] == db["n_nodes"], i
            n = da["n_nodes"]
            for f in ("visit", "value_sum", "reward", "prior", "child_base", "action"):
                assert np.array_equal(da[f][:n], db[f][:n]), (i, f)
            for f in ("minmax", "path", "root_priors"):
                assert np.array_equal(da[f], db[f]), (i, f)
            assert a.philox_position(i) == b.philox_position(i), i
    for x, y in zip(a.root_stats(), b.root_stats()):
        assert torch.equal(x, y)


CASES = [(33, 2, 5, 12, "mt19937"), (33, 2, 5, 12, "philox"),          # fewer actions than lanes; last workgroup: one tree
         (129, 3, 8, 20, "mt19937"), (129, 3, 8, 20, "philox"),        # two policy panels, the second one column wide
         (256, 2, 64, 10, "philox"),                                   # whole panels, 16 workgroups
         (1000, 5, 7, 8, "mt19937"),                                   # 8 panels, the last ragged; T = 3
         (1024, 2, 7, 10, "mt19937"), (1024, 2, 7, 10, "philox"),      # the action limit, T = 3, ragged last workgroup
         (64, 2, 4, 0, "mt19937"),                                     # no rounds: root only
         (64, 2, 4, 1, "mt19937")]                                     # one round


@pytest.mark.parametrize("A,K,B,sims,rng", CASES, ids=[f"A{c[0]}_K{c[1]}_B{c[2]}_s{c[3]}_{c[4]}" for c in CASES])
def test_single_launch_equals_the_stepwise_search(A, K, B, sims, rng, geometry):
    (_, step), (_, single) = _pair(A, K, B, sims, rng)
    assert int(single.root_stats()[0].sum()) == B * sims
    _equal(step, single, B)


@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_single_launch_equals_the_stepwise_search_without_noise(rng, geometry):
    """train=False at A = 129: no Dirichlet noise, the root priors are written by root init."""
    (_, step), (_, single) = _pair(129, 3, 8, 20, rng, train=False)
    assert int(single.root_stats()[0].sum()) == 8 * 20
    _equal(step, single, 8)


def test_more_workgroups_than_compute_units():
    """A = 129, K = 2, 2050 trees, 5 simulations, Philox: 513 workgroups of four trees (the launcher's own choice at this
    batch), the last one with two.  At A > 128 the step-wise heads still run their split geometry here, so equality is exact.  All four root statistics of every tree; trees
    and stream positions of the first and last workgroups and every 97th tree in between."""
    B = 2050
    (_, step), (_, single) = _pair(129, 2, B, 5, "philox")
    assert (single.root_stats()[0].sum(1) == 5).all()
    _equal(step, single, B, trees=sorted(set(range(8)) | set(range(0, B, 97)) | set(range(B - 6, B))))


def test_inactive_trees(geometry):
    """A = 256, 10 trees, 10 simulations; trees 1, 3 and the whole second workgroup (4-7) switched off: the result equals the
    step-wise run with the same mask, the off trees have no visits and their streams stand where they stood before the search."""
    A, B, sims = 256, 10, 10
    active = torch.ones(B, dtype=torch.uint8)
    off = [1, 3, 4, 5, 6, 7]
    active[off] = 0
    active = active.cuda()
    (_, step), (_, single) = _pair(A, 2, B, sims, "mt19937", active=active)
    _equal(step, single, B)
    visits = single.root_stats()[0].cpu()
    on = [i for i in range(B) if i not in off]
    assert (visits[off] == 0).all() and (visits[on].sum(1) == sims).all()
    fresh = _pkg("engine").SearchEngine(B, A, 16, num_simulations=sims, large_actions=True)
    fresh.seed(np.arange(B, dtype=np.uint64) + 7)
    torch.cuda.synchronize()
    for i in off:
        (ka, pa), (kb, pb) = single.get_rng_state(i), fresh.get_rng_state(i)
        assert pa == pb and np.array_equal(ka, kb), i
    fresh.close()


@pytest.mark.parametrize("T", [1.0, 0.0])
def test_act_in_the_tail(T, geometry):
    """A = 129, 8 trees, 12 simulations with act_temperature: actions, policies, child visits, root values and stream positions
    equal the step-wise search followed by act(T)."""
    A, B, sims = 129, 8, 12
    _, heads = _net(A)
    obs, seeds = _obs(B, 9), np.arange(B, dtype=np.uint64) + 21
    outs, engines = [], []
    for single in (False, True):
        mc = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, maxium_action_sample=3, use_graph=False, large_single_launch=single)
        mc.seed(seeds)
        eng = _run(mc, obs, heads, single, act_temperature=T)
        outs.append([t.clone() for t in eng.act(T)])
        torch.cuda.synchronize()
        engines.append(eng)
    for x, y in zip(*outs):
        assert torch.equal(x, y), T
    _equal(engines[0], engines[1], B)


def test_two_consecutive_searches_on_one_object(geometry):
    """A = 64, 6 trees, 10 simulations, twice on the same BatchedMCTS (streams carried over, policy work rows reused): the second
    search equals the step-wise second search."""
    A, B, sims = 64, 6, 10
    _, heads = _net(A)
    seeds = np.arange(B, dtype=np.uint64) + 2
    engines = []
    for single in (False, True):
        mc = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, use_graph=False, large_single_launch=single)
        mc.seed(seeds)
        _run(mc, _obs(B, 31), heads, single)
        engines.append(_run(mc, _obs(B, 32), heads, single))
    _equal(engines[0], engines[1], B)
    assert int(engines[1].root_stats()[0].sum()) == B * sims


def test_refusals():
    """Return code and a message that names smz_search_mlp_large: a per-lane handle, a wide-layout descriptor, a descriptor
    with another S, a two-player handle.  None of them launches anything."""
    lib_mod, eng_mod, mcts_mod = _pkg("_lib"), _pkg("engine"), _pkg("mcts")
    A, S, B = 64, 16, 4
    _, heads = _net(A)
    hidden, policy = (t.clone() for t in heads.initial(_obs(B, 5)))

    def refused(eng, desc, hid=hidden, pol=policy):
        with pytest.raises(lib_mod.SmzError) as err:
            eng.search_mlp_large(desc, heads.packed, hid, pol, train=True)
        assert err.value.code == lib_mod.SMZ_ERR_INVALID and "smz_search_mlp_large" in str(err.value), str(err.value)
        assert eng.last_kernel() == ""

    lane = eng_mod.SearchEngine(B, 4, S, num_simulations=2)
    refused(lane, heads.large_desc, pol=policy[:, :4].contiguous())
    large = eng_mod.SearchEngine(B, A, S, num_simulations=2, large_actions=True)
    wide = lib_mod.MlpDesc(6, A, S, 64, 1)
    assert lib_mod.load().smz_mlp_layout_wide(C.byref(wide)) == 0
    refused(large, wide)
    other_s = eng_mod.SearchEngine(B, A, S + 1, num_simulations=2, large_actions=True)
    refused(other_s, heads.large_desc, hid=torch.zeros(B, S + 1, device="cuda"))
    two = eng_mod.SearchEngine(B, A, S, num_simulations=2, large_actions=True)
    two.set_players(mcts_mod.cycle_values(2, None))
    refused(two, heads.large_desc)
    # the engine that refused still searches
    large.seed(0)
    large.search_mlp_large(heads.large_desc, heads.packed, hidden, policy, train=True)
    visits = large.root_stats()[0]
    torch.cuda.synchronize()
    assert (visits.sum(1) == 2).all() and large.last_kernel().startswith(KERNEL)
    for e in (lane, large, other_s, two):
        e.close()


def test_two_players_search_stepwise_with_the_flag_on():
    """BatchedMCTS(number_of_player=2, large_single_launch=True) at A = 64: the step-wise kernels, the result of the flag off."""
    B = 6
    (_, off), (_, on) = _pair(64, 2, B, 10, "mt19937", number_of_player=2)
    assert on.last_kernel() == ""
    _equal(off, on, B)


def test_other_heads_search_stepwise_without_a_warning():
    """A = 64 with backend="torch" heads and the flag on: step-wise, no warning (_run asserts it), the result of the flag off."""
    B = 6
    (_, off), (_, on) = _pair(64, 2, B, 10, "mt19937", backend="torch")
    assert on.last_kernel() == "" and not hasattr(_net(64, "torch")[1], "large_desc")
    _equal(off, on, B)
