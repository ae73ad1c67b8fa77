"""Large-action handles (smz_create_large_actions: one wavefront per tree, up to 1024 actions) on the GPU.  Every comparison is
exact: the wave-per-tree kernels must reproduce the per-lane kernels on every tree they share (A <= 32) and the oracle
(oracle/smz_oracle.c, numpy's arithmetic restated, 1 .. 1024 actions) above that: here up to 128 actions, in
test_gpu_large_actions_oracle.py from 129 to 1024.  The tests of wider roots in this file check numpy's pairwise sums directly."""
import glob
import os

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

LARGE = sorted("large_actions/" + os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gu.GOLDEN, "large_actions", "*.npz")))
PLAYERS = sorted("players/" + os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gu.GOLDEN, "players", "*.npz"))
                 if "selfplay" not in p)


def _smz():
    import stochastic_muzero_amd as smz
    return smz


def _engine(B, A, S, sims, K, large, philox=False, **kw):
    smz = _smz()
    mode = smz._lib.RNG_PHILOX if philox else smz._lib.RNG_MT19937_NUMPY
    return smz.SearchEngine(B, A, S, num_simulations=sims, maxium_action_sample=K, discount=0.97, root_dirichlet_alpha=0.3,
                            root_exploration_fraction=0.25, rng_mode=mode, large_actions=large, **kw)


def _softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def _heads_tape(B, A, S, sims, seed):
    """Random but fixed network outputs: the root's and one set per simulation (both engines see the same numbers)."""
    g = np.random.default_rng(seed)
    root = (g.standard_normal((B, S)).astype(np.float32), _softmax(3 * g.standard_normal((B, A))))
    steps = [(g.standard_normal((B, S)).astype(np.float32), g.standard_normal(B).astype(np.float32),
              _softmax(3 * g.standard_normal((B, A))), g.standard_normal(B).astype(np.float32)) for _ in range(sims)]
    return root, steps


def _cuda(*xs):
    return [torch.from_numpy(x).cuda() for x in xs]


def _run(eng, root, steps, train=True, fused=False, oracle=None):
    """Root + simulations on one engine; with `oracle` (orc.Tree per tree) the oracle replays and must select alike."""
    h0, p0 = root
    if oracle is not None:           # (no noise override: the device's own gammas must be numpy's)
        for i, t in enumerate(oracle):
            t.root_init(p0[i], hidden=h0[i], train=train)
    eng.root_init(*_cuda(h0, p0), train=train)
    eng.select()
    for s, (h, r, p, v) in enumerate(steps):
        torch.cuda.synchronize()
        if oracle is not None:
            act, br, ph = eng.last_action.cpu().numpy(), eng.branch.cpu().numpy(), eng.parent_hidden.cpu().numpy()
            for i, t in enumerate(oracle):
                _, _, oa, of, oph = t.select(want_hidden=True)
                assert (oa, of) == (act[i], br[i]), f"simulation {s}, tree {i}"
                assert np.array_equal(oph[:ph.shape[1]], ph[i]), f"simulation {s}, tree {i}: parent hidden row"
                t.expand_backup(p[i], v[i], reward=r[i], hidden=h[i])
        if fused and s + 1 < len(steps):
            eng.expand_backup_select(*_cuda(h, r, p, v))
        else:
            eng.expand_backup(*_cuda(h, r, p, v))
            if s + 1 < len(steps):
                eng.select()
    torch.cuda.synchronize()


def _trees_equal(a, b, B):
    for i in range(B):
        da, db = a.dump_tree(i), b.dump_tree(i)
        assert da["n_nodes"] == db["n_nodes"], i
        n = da["n_nodes"]
        for f in ("visit", "value_sum", "reward", "prior", "child_base", "action"):
            assert np.array_equal(da[f][:n], db[f][:n]), (i, f)
        for f in ("minmax", "path", "root_priors"):
            assert np.array_equal(da[f], db[f]), (i, f)
    for x, y in zip(a.root_stats(), b.root_stats()):
        assert torch.equal(x, y)


def _streams_equal(a, b, B):
    for i in range(B):
        if a.cfg.rng_mode == 1:
            assert a.philox_position(i) == b.philox_position(i), i
        else:
            ka, pa = a.get_rng_state(i)
            kb, pb = b.get_rng_state(i)
            ra = np.random.RandomState(0); ra.set_state(("MT19937", ka, pa, 0, 0.0))
            rb = np.random.RandomState(0); rb.set_state(("MT19937", kb, pb, 0, 0.0))
            assert np.array_equal(ra.random_sample(8), rb.random_sample(8)), f"tree {i}: stream position"


def _acts_equal(a, b, T):
    oa, ob = a.act(T), b.act(T)
    torch.cuda.synchronize()
    for x, y in zip(oa, ob):
        assert torch.equal(x, y), T


@pytest.mark.parametrize("philox", [False, True])
@pytest.mark.parametrize("A,K", [(2, 2), (4, 4), (17, 2), (17, 7), (32, 2), (32, 32)])
def test_large_action_handle_equals_the_per_lane_kernels(A, K, philox):
    """A <= 32: an LA handle and an smz_create handle on the same seeds build the same trees, draw the same words and act alike;
    a second search continues the streams."""
    B, S, sims = 256, 8, 30
    root, steps = _heads_tape(B, A, S, sims, seed=A * 100 + K)
    narrow, large = _engine(B, A, S, sims, K, False, philox), _engine(B, A, S, sims, K, True, philox)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 5
    for e in (narrow, large):
        e.seed(seeds)
    _run(narrow, root, steps, fused=True)
    _run(large, root, steps, fused=True)
    _trees_equal(narrow, large, B)
    _streams_equal(narrow, large, B)
    for T in (0.0, 0.5, 1.0):
        _acts_equal(narrow, large, T)
    _run(narrow, root, steps[:10], train=False)
    _run(large, root, steps[:10], train=False)
    _trees_equal(narrow, large, B)
    _streams_equal(narrow, large, B)


@pytest.mark.parametrize("A,K", [(33, 2), (33, 7), (64, 2), (64, 7), (100, 5), (128, 2), (128, 7), (128, 128)])
def test_large_action_handle_equals_the_oracle(A, K):
    """33 <= A <= 128 against the oracle on every tree: selections, parent rows, trees, priors (float64, exact), paths, MinMax,
    stream positions; then act at T in {0, 0.5, 1} and a second search that continues the streams."""
    import orc
    from test_gpu_fullsize_parity import assert_engine_equals_oracle
    B, S, sims = 1024, 8, 50
    root, steps = _heads_tape(B, A, S, sims, seed=A * 1000 + K)
    eng = _engine(B, A, S, sims, K, True)
    seeds = np.arange(B, dtype=np.uint64) + 11
    eng.seed(seeds)
    cfg = orc.make_cfg(A, K, S, sims, discount=0.97, alpha=0.3, frac=0.25)
    trees = []
    for i in range(B):
        t = orc.Tree(cfg)
        t.seed(int(seeds[i]))
        trees.append(t)
    _run(eng, root, steps, oracle=trees)
    assert_engine_equals_oracle(eng, trees, sims, prior_rtol=0)
    for T in (0.0, 0.5, 1.0):
        act, pol, cv, rv = (x.cpu().numpy() for x in eng.act(T))
        for i, t in enumerate(trees):
            oa, opol, ocv, orv = t.act(T)
            assert act[i] == oa and np.array_equal(pol[i], opol) and np.array_equal(cv[i], ocv) and rv[i] == orv, (T, i)
    root2, steps2 = _heads_tape(B, A, S, 12, seed=A + K)
    _run(eng, root2, steps2, oracle=trees)
    assert_engine_equals_oracle(eng, trees, 12, prior_rtol=0)


@pytest.mark.parametrize("A,K", [(256, 2), (256, 256), (1000, 2), (1024, 3)])
def test_wide_roots_follow_numpys_pairwise_sums(A, K):
    """Above numpy's 128-element summation block, against numpy itself: the root priors are numpy's (policy + 1e-12) / sum with numpy's pairwise float32 sum,
    the visit-policy of act is numpy's, every simulation adds one visit, graph-free and fused runs agree."""
    B, S, sims = 64, 8, 12
    root, steps = _heads_tape(B, A, S, sims, seed=A + 3 * K)
    a, b = _engine(B, A, S, sims, K, True), _engine(B, A, S, sims, K, True)
    _run(a, root, steps, train=False)
    _run(b, root, steps, train=False, fused=True)
    _trees_equal(a, b, B)
    p = root[1] + np.float32(1e-12)
    want = np.stack([p[i] / p[i].sum() for i in range(B)])          # 1-D float32 sums: numpy's pairwise order
    visits, priors, rv, _ = (x.cpu().numpy() for x in a.root_stats())
    for i in range(B):
        d = a.dump_tree(i)
        assert np.array_equal(d["prior"][1:1 + A], want[i]), i
        assert np.array_equal(priors[i], want[i].astype(np.float64)), i
        assert visits[i].sum() == sims and d["visit"][0] == sims, i
    act, pol, cv, _ = (x.cpu().numpy() for x in a.act(1.0))
    vis = visits.astype(np.float64)
    for i in range(B):
        wp = vis[i] / vis[i].sum()
        assert np.array_equal(pol[i], wp) and np.array_equal(cv[i], wp), i
        assert 0 <= act[i] < A and visits[i][act[i]] > 0, i


@pytest.mark.parametrize("A", [2, 17, 32])
def test_philox_large_action_handle_equals_narrow(A):
    B, S, sims, K = 128, 8, 25, 2
    root, steps = _heads_tape(B, A, S, sims, seed=A)
    n, l = _engine(B, A, S, sims, K, False, True), _engine(B, A, S, sims, K, True, True)
    _run(n, root, steps)
    _run(l, root, steps)
    _trees_equal(n, l, B)
    _streams_equal(n, l, B)


@pytest.mark.parametrize("philox", [False, True])
def test_batched_mcts_at_100_actions_graph_and_no_graph(philox, recwarn):
    """BatchedMCTS end to end at A = 100 with a fresh mlp_model's HIP heads (A + S <= 128): an LA engine, no single-launch
    attempt, and the captured graph equals the eager step-wise run."""
    from importlib import import_module
    mcts_mod, model_mod = import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.model")
    A, B, sims = 100, 256, 20
    torch.manual_seed(1)
    m = model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=6, action_space_dimensions=A,
                         state_space_dimensions=16, hidden_layer_dimensions=64, number_of_hidden_layer=1)
    heads = m.heads("cuda:0")
    obs = torch.randn(B, 6, generator=torch.Generator().manual_seed(3)).cuda()
    out = []
    for use_graph in (True, False):
        mc = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, use_graph=use_graph,
                             rng_mode="philox" if philox else "mt19937")
        mc.seed(np.arange(B, dtype=np.uint64))
        eng = mc.run(obs, heads, train=True)
        assert eng.large_actions and eng.A == A
        v, p, rv, cr = (x.clone() for x in eng.root_stats())
        out.append((v, p, rv, eng.act(1.0)[0].clone()))
        assert int(v.sum()) == B * sims
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert not [w for w in recwarn if "single-launch" in str(w.message)]


def test_refusals():
    smz = _smz()
    C = smz._lib
    lib = C.load()
    import ctypes
    for A in (0, 1025):
        cfg = C.Config(4, A, 2, 8, 10, 19652, 1.25, 0.95, 0.25, 0.25, 0, torch.cuda.current_device())
        h = ctypes.c_void_p()
        assert lib.smz_create_large_actions(ctypes.byref(cfg), ctypes.byref(h)) == C.SMZ_ERR_INVALID
    cfg = C.Config(4, 33, 2, 8, 10, 19652, 1.25, 0.95, 0.25, 0.25, 0, torch.cuda.current_device())
    h = ctypes.c_void_p()
    assert lib.smz_create(ctypes.byref(cfg), ctypes.byref(h)) == C.SMZ_ERR_INVALID
    eng = _engine(4, 2, 8, 10, 2, True)
    null = None
    assert lib.smz_search_mlp(eng.h, null, null, null, 1, null) == C.SMZ_ERR_TOO_LARGE
    assert lib.smz_search_mlp_act(eng.h, null, null, null, 1, 1.0, null, null, null, null, null, null) == C.SMZ_ERR_TOO_LARGE
    assert lib.smz_search_mlp_act_cartpole(eng.h, null, null, 1, 1.0, null, null, null, null, null, null, null) == C.SMZ_ERR_TOO_LARGE
    assert lib.smz_search_vision(eng.h, null, null, null, null, 1, null) == C.SMZ_ERR_TOO_LARGE
    assert lib.smz_enable_stats(eng.h, 1) == C.SMZ_ERR_TOO_LARGE
    assert b"large-action" in lib.smz_last_error()


# ---- fixtures written by the reference (tests/golden: the narrow corpus, players/, large_actions/) on large-action handles ----
def _la_engine(cfg, A, S, sims, B):
    return _smz().SearchEngine(num_trees=B, num_actions=A, hidden_size=S, num_simulations=sims,
                               maxium_action_sample=int(cfg["maxium_action_sample"]), pb_c_base=int(cfg["pb_c_base"]),
                               pb_c_init=float(cfg["pb_c_init"]), discount=float(cfg["discount"]),
                               root_dirichlet_alpha=float(cfg["root_dirichlet_alpha"]),
                               root_exploration_fraction=float(cfg["root_exploration_fraction"]), large_actions=True)


def drive(name, make_engine=_la_engine, fused=False):
    """Every case of a search fixture as one batch on an engine from `make_engine`; the device must ask the heads for what the
    reference asked (branch, action, parent row, one-hot input) at every simulation.  Multi-player fixtures (cfg
    number_of_player / custom_loop) hand their turn cycle and root players to the engine."""
    from importlib import import_module
    import gpu_harness as gh
    cfg, data = gu.load(name)
    B, A, S = data["seed"].shape[0], data["root_policy"].shape[-1], data["root_hidden"].shape[-1]
    sims = int(cfg["num_simulations"])
    eng = make_engine(cfg, A, S, sims, B)
    if int(cfg.get("number_of_player", 1) or 1) > 1 or cfg.get("custom_loop") is not None:
        mcts = import_module("stochastic-muzero_amd.mcts")
        cyc = mcts.cycle_values(number_of_player=int(cfg.get("number_of_player", 1)), custom_loop=cfg.get("custom_loop"))
        eng.set_players(cyc, root_player=data["root_to_play"])
    eng.seed(data["seed"].astype(np.uint64))
    eng.root_init(gh.dev(data["root_hidden"]), gh.dev(data["root_policy"]), train=bool(data["train"][0]))
    if sims > 0:
        ph, la, br, xin = eng.select()
    for s in range(sims):
        torch.cuda.synchronize()
        assert np.array_equal(br.cpu().numpy(), data["tape_branch"][:, s].astype(np.uint8)), f"sim {s}: branch"
        assert np.array_equal(la.cpu().numpy(), data["tape_action"][:, s]), f"sim {s}: last action"
        assert np.array_equal(ph.cpu().numpy()[:, :S], data["tape_hidden_in"][:, s]), f"sim {s}: parent hidden"
        x = xin.cpu().numpy()
        assert np.array_equal(x[:, :S], data["tape_hidden_in"][:, s])
        assert np.array_equal(x[:, S:], np.eye(A, dtype=np.float32)[data["tape_action"][:, s]]), f"sim {s}: one-hot"
        args = (gh.dev(data["tape_hidden_out"][:, s]), gh.dev(data["tape_reward"][:, s]), gh.dev(data["tape_policy"][:, s]),
                gh.dev(data["tape_value"][:, s]))
        if fused and s + 1 < sims:
            ph, la, br, xin = eng.expand_backup_select(*args)
        else:
            eng.expand_backup(*args)
            if s + 1 < sims:
                ph, la, br, xin = eng.select()
    torch.cuda.synchronize()
    return eng, cfg, data


def _check_acts(eng, data, sims):
    """Game.policy_step / store_search_statistics at every temperature of the fixture, each from the search's stream state."""
    eng.snapshot_rng()
    for T in gu.TEMPERATURES:
        k = f"T{T}"
        if k + "_action" not in data:
            continue
        eng.restore_rng()
        action, policy, child_visits, root_value = (x.cpu().numpy() for x in eng.act(T))
        assert np.array_equal(action, data[k + "_action"]), T
        assert np.array_equal(policy, data[k + "_policy"]), T
        assert np.array_equal(child_visits, data[k + "_child_visits"]), T
        assert np.array_equal(root_value, data[k + "_root_value"]), T
        for i in range(data["seed"].shape[0]):
            key, pos = eng.get_rng_state(i)
            rs = np.random.RandomState(0); rs.set_state(("MT19937", key, pos, 0, 0.0))
            assert rs.random_sample() == data[k + "_probe"][i], (T, i)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", LARGE)
def test_reference_fixtures_above_32_actions(name, fused):
    """The reference's own searches with 33 .. 1024 actions (tools/gen_golden_large_actions.py): trees, device-drawn Dirichlet
    priors (float64, exact), paths, MinMax, stream positions, and the act outputs at every temperature."""
    import gpu_harness as gh
    eng, cfg, data = drive(name, fused=fused)
    assert eng.large_actions
    gh.check_fixture_outputs(eng, cfg, data, prior_exact=False)
    _check_acts(eng, data, int(cfg["num_simulations"]))


@pytest.mark.parametrize("name", gu.SEARCH_FIXTURES + PLAYERS)
def test_narrow_corpus_on_large_action_handles(name):
    """Every search fixture of the per-lane kernels (and the multi-player ones, with their turn cycles) replayed on a
    large-action handle: the wave-per-tree kernels against the whole existing corpus."""
    import gpu_harness as gh
    eng, cfg, data = drive(name, fused=name.endswith("sims50"))
    assert eng.large_actions
    gh.check_fixture_outputs(eng, cfg, data, prior_exact=False)
    _check_acts(eng, data, int(cfg["num_simulations"]))


@pytest.mark.parametrize("A", [256, 1000])
def test_priors_only_act_follows_numpys_float64_pairwise_sum(A):
    """No simulation: act builds its policy and child visits from the float64 root priors, whose sums above 128 entries are
    numpy's pairwise ones."""
    B, S = 32, 8
    root, _ = _heads_tape(B, A, S, 0, seed=A)
    eng = _engine(B, A, S, 0, 2, True)
    eng.root_init(*_cuda(*root), train=True)
    _, priors, _, _ = (x.cpu().numpy() for x in eng.root_stats())
    action, policy, cv, _ = (x.cpu().numpy() for x in eng.act(1.0))
    for i in range(B):
        want = priors[i] / priors[i].sum()
        assert np.array_equal(policy[i], want) and np.array_equal(cv[i], want), i
        assert 0 <= action[i] < A
