"""smz_search_mlp_players: the whole search of every tree of a multi-player handle in one launch
(csrc/smz_mlp_players_search.hip), opt-in through BatchedMCTS(players_single_launch=True), against the step-wise multi-player
kernels with the same HipMlpHeads.  The step-wise path is pinned to the reference's own trees (test_gpu_players.py); the single
launch calls the same device functions (expand_backup_tree<..., MP>, select_tree, the row bodies of the head kernels, compiled
with the same flags) on the same streams, so every comparison here is np.array_equal: there is no tolerance in this file."""
import os
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu
import mlp_reference as mr
from search_helpers import _lib, _pkg, _states

pytestmark = pytest.mark.gpu

FIELDS = ("visit", "value_sum", "reward", "child_base", "action", "minmax")
KW = dict(discount=0.999, root_exploration_fraction=0.1)
CYCLES = {"two": dict(number_of_player=2), "three": dict(number_of_player=3), "loop": dict(custom_loop="1>2>1>3")}


_CACHE = {}


def _ckpt421():
    """(model, HipMlpHeads) of the reference's checkpoint 421 (S 31, H 64, A 2), built once."""
    if "ckpt421" not in _CACHE:
        model = _pkg("model").Muzero.from_arrays(os.path.join(gu.GOLDEN, "weights_ckpt421.npz"))
        heads = model.heads("cuda:0")
        assert type(heads).__name__ == "HipMlpHeads"
        _CACHE["ckpt421"] = (model, heads)
    return _CACHE["ckpt421"]


def _obs(B, dim=4):
    return torch.from_numpy(np.random.RandomState(1).uniform(-0.05, 0.05, (B, dim)).astype(np.float32)).cuda()


def _collect(e, rng, trees, act=True):
    """Everything "equal" means: root_stats, act(1.0), the dumped trees and the per-tree stream positions (after the act)."""
    out = [t.clone() for t in e.root_stats()]
    if act:
        out += [t.clone() for t in e.act(1.0)]
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in out]
    dumps = [{f: np.array(d[f]) for f in FIELDS} for d in (e.dump_tree(i) for i in trees)]
    return out, dumps, _states(e, rng, trees)


def _same(a, b, rng, rows=None):
    for x, y in zip(a[0], b[0]):
        assert x.dtype == y.dtype
        assert np.array_equal(x if rows is None else x[rows], y if rows is None else y[rows])
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        for f in FIELDS:
            assert np.array_equal(x[f], y[f]), f
    for x, y in zip(a[2], b[2]):
        if rng == "philox":
            assert x == y
        else:
            assert np.array_equal(x[0], y[0]) and x[1] == y[1]


def _searcher(B, sims, rng, flag, cyc, **kw):
    m = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, use_graph=False, rng_mode=rng, players_single_launch=flag, **KW, **cyc, **kw)
    m.seed(np.arange(B, dtype=np.uint64))
    return m


def _check_path(m, e, flag):
    if flag:
        assert m._single is True and e.last_kernel().startswith("k_search_mlp_players<"), (m._single, e.last_kernel())
    else:
        assert m._single is None and e.last_kernel() == ""


def _pair_search(heads, B, sims, rng, flag, cyc, obs, K=2):
    """Two searches on one engine: root players arange(B) % 5 (beyond every cycle length: the kernel takes the modulo) as a host
    array, then, on other observations, as a device tensor.  The first search's root statistics and the second's everything."""
    m = _searcher(B, sims, rng, flag, cyc, maxium_action_sample=K)
    to_play = (np.arange(B) % 5).astype(np.int32)
    e = m.run(obs, heads, train=True, to_play=to_play)
    first = [t.clone() for t in e.root_stats()]
    e = m.run(obs + 0.01, heads, train=True, to_play=torch.from_numpy(to_play[::-1].copy()).cuda())
    _check_path(m, e, flag)
    res = _collect(e, rng, range(B))
    res[0].extend(t.cpu().numpy() for t in first)
    e.close()
    return res


def _stepwise(key, heads, B, sims, rng, cyc, obs, K=2):
    """The step-wise side of a case, computed once and shared."""
    if key not in _CACHE:
        _CACHE[key] = _pair_search(heads, B, sims, rng, False, cyc, obs, K)
    return _CACHE[key]


# ---- 1. single launch == step-wise ----------------------------------------------------------------------------------------------
# 50 simulations: paths deeper than the backup's 8-record chunk and than every cycle length.  B = 68 and 515 leave partly filled
# wavefronts' workgroups: 68 = 8 workgroups of 8 one-tree wavefronts + 4 wavefronts; 515 likewise with 3.
@pytest.mark.parametrize("B", [1, 68, 515])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("cycle", list(CYCLES))
def test_single_launch_equals_stepwise(cycle, rng, B):
    _, heads = _ckpt421()
    obs = _obs(B)
    step = _stepwise(("t1", cycle, rng, B), heads, B, 50, rng, CYCLES[cycle], obs)
    one = _pair_search(heads, B, 50, rng, True, CYCLES[cycle], obs)
    assert (one[0][0].sum(1) == 50).all()
    _same(one, step, rng)


# ---- 6. not vacuous: two players search other trees than one ------------------------------------------------------------------
def test_two_players_search_other_trees_than_one_player():
    _, heads = _ckpt421()
    B = 68
    obs = _obs(B)
    two = _pair_search(heads, B, 50, "mt19937", True, CYCLES["two"], obs)
    m = _searcher(B, 50, "mt19937", False, dict(number_of_player=1))
    m.run(obs, heads, train=True)
    e = m.run(obs + 0.01, heads, train=True)
    assert e.last_kernel().startswith("k_search_mlp<")
    cv1 = e.act(1.0)[2].cpu().numpy()
    assert cv1.shape == two[0][6].shape
    assert (cv1 != two[0][6]).any(axis=1).sum() >= 1          # child_visits of at least one tree


# ---- 2. the result does not depend on the trees per wavefront -------------------------------------------------------------------
@pytest.mark.parametrize("tpw", [1, 5])
def test_trees_per_wavefront_do_not_change_the_search(tpw, monkeypatch):
    """68 trees, one per wavefront and five per wavefront (14 wavefronts, the last with three trees)."""
    monkeypatch.setenv("SMZ_PLAYERS_SEARCH_TPW", str(tpw))
    _, heads = _ckpt421()
    B = 68
    obs = _obs(B)
    step = _stepwise(("t1", "two", "mt19937", B), heads, B, 50, "mt19937", CYCLES["two"], obs)
    one = _pair_search(heads, B, 50, "mt19937", True, CYCLES["two"], obs)
    _same(one, step, "mt19937")


# ---- 3. masks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_masked_trees_are_left_alone(rng):
    """515 trees (one per wavefront), every third switched off after one full search, and trees 24..31 as well (a whole workgroup,
    so every one of its wavefronts is idle): the searched trees equal the step-wise search under the same mask; the dumped trees
    and stream positions of the others are what they were before the launch."""
    _, heads = _ckpt421()
    B, sims = 515, 20
    obs = _obs(B)
    active = torch.ones(B, dtype=torch.uint8)
    active[::3] = 0
    active[24:32] = 0
    off, on = [int(i) for i in np.flatnonzero(active.numpy() == 0)], [int(i) for i in np.flatnonzero(active.numpy())]
    active = active.cuda()
    to_play = (np.arange(B) % 5).astype(np.int32)
    res = []
    for flag in (True, False):
        m = _searcher(B, sims, rng, flag, CYCLES["three"])
        e = m.run(obs, heads, train=True, to_play=to_play)
        torch.cuda.synchronize()
        before = ([{f: np.array(d[f]) for f in FIELDS} for d in (e.dump_tree(i) for i in off)], _states(e, rng, off))
        m.set_active(active)
        e = m.run(obs + 0.01, heads, train=True, to_play=to_play)
        _check_path(m, e, flag)
        got = _collect(e, rng, on)
        after = ([{f: np.array(d[f]) for f in FIELDS} for d in (e.dump_tree(i) for i in off)], _states(e, rng, off))
        _same(([], *before), ([], *after), rng)
        res.append(got)
        e.close()
    _same(res[0], res[1], rng, rows=on)


# ---- 4. run-time A below the bucket, run-time K ---------------------------------------------------------------------------------
# (obs, A, S, H, L) -> bucket
SHAPES = [((6, 3, 15, 32, 1), 4), ((10, 7, 15, 32, 1), 8), ((12, 9, 21, 32, 0), 16), ((8, 20, 15, 32, 1), 32)]


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("shape,bucket", SHAPES)
def test_action_counts_below_their_bucket_and_run_time_k(shape, bucket, K):
    key = ("net",) + shape
    if key not in _CACHE:
        heads = mr.fresh_net(*shape, seed=0).heads("cuda:0")
        assert type(heads).__name__ == "HipMlpHeads"
        _CACHE[key] = heads
    heads = _CACHE[key]
    B, sims = 37, 12
    obs = _obs(B, shape[0])
    m = _searcher(B, sims, "mt19937", True, CYCLES["two"], maxium_action_sample=K)
    e = m.run(obs, heads, train=True, to_play=(np.arange(B) % 5).astype(np.int32))
    assert e.last_kernel() == "k_search_mlp_players<%d, %d, false>" % (bucket, 2 if K == 2 else 0), e.last_kernel()
    e.close()
    step = _pair_search(heads, B, sims, "mt19937", False, CYCLES["two"], obs, K)
    one = _pair_search(heads, B, sims, "mt19937", True, CYCLES["two"], obs, K)
    assert (one[0][0].sum(1) == sims).all()
    _same(one, step, "mt19937")


# ---- 5. a cycle of alike players is the one-player single launch ------------------------------------------------------------------
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_alike_players_equal_the_one_player_single_launch(rng):
    _, heads = _ckpt421()
    B, sims = 130, 30
    obs = _obs(B)
    res = []
    for cyc in (dict(custom_loop="1>1"), dict(number_of_player=1)):
        multi = "custom_loop" in cyc
        m = _searcher(B, sims, rng, multi, cyc)
        e = m.run(obs, heads, train=True, **(dict(to_play=np.arange(B) % 2) if multi else {}))
        assert m._single is True
        assert e.last_kernel().startswith("k_search_mlp_players<" if multi else "k_search_mlp<"), e.last_kernel()
        res.append(_collect(e, rng, range(B)))
        e.close()
    _same(res[0], res[1], rng)


# ---- 7. act in the launch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1.0, 0.25, 0.0])
def test_act_in_the_tail_of_the_launch(T):
    _, heads = _ckpt421()
    B, sims = 68, 20
    obs = _obs(B)
    to_play = (np.arange(B) % 5).astype(np.int32)
    res = []
    for flag in (True, False):
        m = _searcher(B, sims, "mt19937", flag, CYCLES["two"])
        e = m.run(obs, heads, train=True, act_temperature=T, to_play=to_play)
        _check_path(m, e, flag)
        assert e._act_done == (T if flag else None)              # (the step-wise search leaves the action selection to act())
        out = [t.clone() for t in e.act(T)]
        torch.cuda.synchronize()
        res.append(([t.cpu().numpy() for t in out], [], _states(e, "mt19937", range(B))))
        e.close()
    _same(res[0], res[1], "mt19937")


# ---- 8. refusals and fallback -----------------------------------------------------------------------------------------------------
def test_refusals():
    lib, eng_mod = _lib(), _pkg("engine")
    _, heads = _ckpt421()
    B, sims = 16, 4
    obs = _obs(B)
    cyc = _pkg("mcts").cycle_values(2, None)
    one = eng_mod.SearchEngine(B, heads.A, heads.S, num_simulations=sims)
    with pytest.raises(lib.SmzError, match="use smz_search_mlp$") as err:
        one.search_mlp_players(heads.desc, heads.weights, obs)
    assert err.value.code == lib.SMZ_ERR_INVALID
    one.close()
    big = eng_mod.SearchEngine(B, heads.A, heads.S, num_simulations=sims, large_actions=True)
    big.set_players(cyc)
    with pytest.raises(lib.SmzError) as err:
        big.search_mlp_players(heads.desc, heads.weights, obs)
    assert err.value.code == lib.SMZ_ERR_TOO_LARGE
    big.close()
    # a descriptor smz_mlp_layout rejects: the wide config-434 shape (HipMlpTileHeads)
    wide = _pkg("model").Muzero.from_arrays(os.path.join(gu.GOLDEN, "weights_cfg434shape.npz")).heads("cuda:0")
    assert type(wide).__name__ == "HipMlpTileHeads"
    e = eng_mod.SearchEngine(B, wide.A, wide.S, num_simulations=sims)
    e.set_players(cyc)
    with pytest.raises(lib.SmzError) as err:
        e.search_mlp_players(wide.wide_desc, wide.packed, obs)
    assert err.value.code == lib.SMZ_ERR_INVALID
    e.close()
    two = eng_mod.SearchEngine(B, heads.A, heads.S, num_simulations=sims)
    two.set_players(cyc)
    # the one-player entry point still refuses the handle
    with pytest.raises(lib.SmzError, match="multi-player") as err:
        two.search_mlp(heads.desc, heads.weights, obs)
    assert err.value.code == lib.SMZ_ERR_INVALID
    # no instrumented variant
    two.enable_stats(True)
    with pytest.raises(lib.SmzError) as err:
        two.search_mlp_players(heads.desc, heads.weights, obs)
    assert err.value.code == lib.SMZ_ERR_INVALID
    two.enable_stats(False)
    two.seed(0)
    two.search_mlp_players(heads.desc, heads.weights, obs)
    visits = two.root_stats()[0]
    torch.cuda.synchronize()
    assert (visits.cpu().numpy().sum(1) == sims).all()
    two.close()


@pytest.mark.parametrize("why", ["tpw65", "lds"])
def test_outside_the_limits_warns_once_and_searches_stepwise(why, monkeypatch):
    """65 trees per wavefront, or 600 simulations (path records of 8 wavefronts beside the ~100 KB weight image: above 160 KB):
    SMZ_ERR_TOO_LARGE from the entry point; BatchedMCTS says so once over two runs and gives the step-wise result."""
    lib = _lib()
    _, heads = _ckpt421()
    B, sims = (68, 8) if why == "tpw65" else (2, 600)
    if why == "tpw65":
        monkeypatch.setenv("SMZ_PLAYERS_SEARCH_TPW", "65")
    obs = _obs(B)
    res = []
    for flag in (True, False):
        m = _searcher(B, sims, "mt19937", flag, CYCLES["two"])
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for _ in range(2):
                e = m.run(obs, heads, train=True, to_play=np.arange(B) % 2)
        assert m._single is (False if flag else None) and e.last_kernel() == ""
        assert len([w for w in seen if "single-launch multi-player search is outside its limits" in str(w.message)]) == (1 if flag else 0)
        if flag:
            with pytest.raises(lib.SmzError) as err:
                e.search_mlp_players(heads.desc, heads.weights, obs)
            assert err.value.code == lib.SMZ_ERR_TOO_LARGE
        res.append(_collect(e, "mt19937", range(B)))
        e.close()
    _same(res[0], res[1], "mt19937")


# ---- 9. the loops -----------------------------------------------------------------------------------------------------------------
def test_play_games_and_reanalyse_give_the_same_data():
    envs_mod, sp, mcts = _pkg("envs"), _pkg("selfplay"), _pkg("mcts")
    model, heads = _ckpt421()
    B, T, limit = 64, 6, 3
    chunks, re = [], []
    for flag in (True, False):
        env = envs_mod.CartPoleVec(B, "cuda:0", seed=4, on_end="reset", limit=limit)
        env.reset()
        m = _searcher(B, 8, "mt19937", flag, CYCLES["two"])
        chunk = sp.play_games(env, heads, m, 1.0, T)
        torch.cuda.synchronize()
        _check_path(m, m.engine, flag)
        chunks.append(chunk)
    assert torch.equal(chunks[0].data, chunks[1].data)
    arrays = sp.chunk_to_records(chunks[0], None, 2, 0.999, td_steps=4, limit_of_game_play=limit, after_end="new_game",
                                 keep_partial=False)
    assert len(arrays) > 0
    for flag in (True, False):
        m = mcts.BatchedMCTS(128, num_simulations=8, use_graph=False, number_of_player=2, players_single_launch=flag, **KW)
        m.seed(np.arange(128, dtype=np.uint64))
        re.append(sp.reanalyse_replay_records(arrays, model, m, "cuda:0", temperature=1.0, train=True, td_steps=4))
        _check_path(m, m.engine, flag)
    assert len(re[0]) == len(re[1]) > 0
    for ga, gb in zip(*re):
        assert ga.game_length == gb.game_length
        assert np.array_equal(np.array(ga.policies), np.array(gb.policies))
        assert np.array_equal(np.array(ga.child_visits), np.array(gb.child_visits))
        assert np.array_equal(np.array(ga.root_values, np.float32), np.array(gb.root_values, np.float32))
        assert np.array_equal(np.array(ga.rewards, np.float64), np.array(gb.rewards, np.float64))
