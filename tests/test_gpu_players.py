"""Multi-player searches on the MI355X (number_of_player > 1, custom_loop): the step-wise kernels' signed backup against the
reference's own trees (tests/golden/players/*.npz, tools/gen_golden_players.py), through the engine, the reference-shaped
facade and its play_game, BatchedMCTS (graph replays with the root players changed in between), the batched self-play
and reanalyse loops; and the invariance of a cycle whose players are all alike ("1>1") against the single-player kernels."""
import glob
import os
import random
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as gu
import gpu_harness as gh
import seam_harness as sh

pytestmark = pytest.mark.gpu

PLAYERS = sorted("players/" + os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gu.GOLDEN, "players", "*.npz")))
SEARCHES = [n for n in PLAYERS if "selfplay" not in n]
GAME = "players/selfplay421_p2_sims10_T1"


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _cycle(cfg):
    return dict(number_of_player=int(cfg.get("number_of_player", 1)), custom_loop=cfg.get("custom_loop"))


def _hyper(cfg, **kw):
    return dict(pb_c_base=int(cfg["pb_c_base"]), pb_c_init=float(cfg["pb_c_init"]), discount=float(cfg["discount"]),
                root_dirichlet_alpha=float(cfg["root_dirichlet_alpha"]), root_exploration_fraction=float(cfg["root_exploration_fraction"]),
                num_simulations=int(cfg["num_simulations"]), maxium_action_sample=int(cfg["maxium_action_sample"]), **_cycle(cfg), **kw)


def _drive_players(name, fused):
    """gpu_harness.drive_fixture with the fixture's turn cycle and root players handed to the engine."""
    cfg, data = gu.load(name)
    B, A, S = data["seed"].shape[0], data["root_policy"].shape[-1], data["root_hidden"].shape[-1]
    sims = int(cfg["num_simulations"])
    eng = gh.make_engine(cfg, A, S, sims, B)
    eng.set_players(_pkg("mcts").cycle_values(**_cycle(cfg)), root_player=data["root_to_play"])
    eng.seed(data["seed"].astype(np.uint64))
    eng.root_init(gh.dev(data["root_hidden"]), gh.dev(data["root_policy"]), train=bool(data["train"][0]))
    ph, la, br, _ = eng.select()
    for s in range(sims):
        torch.cuda.synchronize()
        assert np.array_equal(br.cpu().numpy(), data["tape_branch"][:, s].astype(np.uint8)), f"sim {s}: branch"
        assert np.array_equal(la.cpu().numpy(), data["tape_action"][:, s]), f"sim {s}: last action"
        assert np.array_equal(ph.cpu().numpy()[:, :S], data["tape_hidden_in"][:, s]), f"sim {s}: parent hidden"
        args = (gh.dev(data["tape_hidden_out"][:, s]), gh.dev(data["tape_reward"][:, s]), gh.dev(data["tape_policy"][:, s]),
                gh.dev(data["tape_value"][:, s]))
        if fused and s + 1 < sims:
            ph, la, br, _ = eng.expand_backup_select(*args)
        else:
            eng.expand_backup(*args)
            if s + 1 < sims:
                ph, la, br, _ = eng.select()
    torch.cuda.synchronize()
    return eng, cfg, data


# ---- (a) the engine, step by step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", SEARCHES)
def test_engine_reproduces_the_references_multi_player_trees(name, fused):
    eng, cfg, data = _drive_players(name, fused)
    gh.check_fixture_outputs(eng, cfg, data, prior_exact=False)


def test_single_launch_refuses_a_multi_player_handle():
    lib = _pkg("_lib")
    heads = _pkg("model").Muzero.from_arrays(os.path.join(gu.GOLDEN, "weights_ckpt421.npz")).heads("cuda:0")
    eng = _pkg("engine").SearchEngine(64, 2, 31, num_simulations=10, discount=0.999, root_exploration_fraction=0.1)
    eng.seed(0)
    obs = torch.zeros(64, 4, dtype=torch.float32, device="cuda:0")
    eng.search_mlp(heads.desc, heads.weights, obs)            # single-player handle: fine
    eng.set_players([0.0, 1.0])
    for call in (lambda: eng.search_mlp(heads.desc, heads.weights, obs),
                 lambda: eng.search_mlp(heads.desc, heads.weights, obs, act_temperature=1.0)):
        with pytest.raises(lib.SmzError) as err:
            call()
        assert err.value.code == lib.SMZ_ERR_INVALID and "multi-player" in str(err.value)
    with pytest.raises(lib.SmzError):
        eng.set_players(np.arange(33, dtype=np.float32))
    eng.set_players([0.0])                                    # one player again: the single launch is back
    eng.search_mlp(heads.desc, heads.weights, obs)
    torch.cuda.synchronize()


# ---- (b) the reference-shaped facade and play_game ---------------------------------------------------------------------------
def _node_to_play(root, child_base, n):
    out = np.full(n, -1, np.int64)
    stack = [(root, 0)]
    while stack:
        node, i = stack.pop()
        out[i] = node.to_play
        for j, c in enumerate(node.children.values()):
            stack.append((c, int(child_base[i]) + j))
    return out


@pytest.mark.parametrize("name", SEARCHES)
def test_facade_searches_like_the_reference(name):
    cfg, data = gu.load(name)
    m = _pkg("mcts").Monte_carlo_tree_search(**_hyper(cfg))
    tape = sh.TapePlayer(data)
    A = data["root_policy"].shape[-1]
    for i in range(data["seed"].shape[0]):
        m.cycle.global_count = int(data["root_to_play"][i])
        np.random.seed(int(data["seed"][i]))
        root = m.run(observation=torch.from_numpy(data["obs"][i][None].copy()), model=tape, train=bool(data["train"][i]))
        assert np.random.random_sample() == data["probe"][i]
        kids = list(root.children.values())
        assert [c.visit_count for c in kids] == list(data["root_visits"][i])
        assert root.to_play == int(data["root_to_play"][i])
        n = data["tree_to_play"][i].size
        assert np.array_equal(_node_to_play(root, data["tree_child_base"][i], n), data["tree_to_play"][i])
        assert np.float32(sum(c.value_sum for c in kids if c.visit_count)) == np.float32(
            sum(data["tree_value_sum"][i][1:1 + A][data["root_visits"][i] > 0]))


def test_play_game_replays_the_references_two_player_game():
    sp = _pkg("selfplay")
    cfg, data = gu.load(GAME)
    search = _pkg("mcts").Monte_carlo_tree_search(**_hyper(cfg))
    roots = []
    run = search.run
    search.run = lambda **kw: (roots.append(search.cycle.global_count), run(**kw))[1]
    random.seed(int(data["seed"]))
    np.random.seed(int(data["seed"]))
    game = _pkg("game").Game(gym_env=sh.MathCartPole(), discount=0.999, limit_of_game_play=int(data["limit"]), observation_dimension=4,
                             action_dimension=2, rgb_observation=False, action_map=[0, 1], priority_scale=0.5)
    g = sp.play_game(environment=game, model=sh.TapePlayer(data), monte_carlo_tree_search=search,
                     temperature=float(data["temperature"]), replay_buffer=sh.FakeBuffer())
    sh.assert_game_equals(g, data)
    assert np.random.random_sample() == data["probe"]
    assert roots == list(data["root_to_play"]) and search.cycle.global_count == 0      # global_reset at the game's end


# ---- (c) BatchedMCTS over many trees, graph replays --------------------------------------------------------------------------
class _TapeHeads:
    """Heads that hand every tree the recorded network outputs of fixture case `case_of[tree]` (device buffers rewritten in
    place, so a captured graph replays with the new contents)."""
    wants_mlp_input, wants_parent_hidden = False, False

    def __init__(self, data, B):
        sims, S = data["tape_value"].shape[1], data["root_hidden"].shape[-1]
        A = data["root_policy"].shape[-1]
        self.d, self.B, self.s = data, B, 0
        dev = "cuda:0"
        self.h0 = torch.empty(B, S, device=dev)
        self.p0 = torch.empty(B, A, device=dev)
        self.hid = torch.empty(sims, B, S, device=dev)
        self.rew = torch.empty(sims, B, device=dev)
        self.pol = torch.empty(sims, B, A, device=dev)
        self.val = torch.empty(sims, B, device=dev)

    def load(self, case_of):
        d = self.d
        self.h0.copy_(torch.from_numpy(d["root_hidden"][case_of]))
        self.p0.copy_(torch.from_numpy(d["root_policy"][case_of]))
        self.hid.copy_(torch.from_numpy(np.ascontiguousarray(d["tape_hidden_out"][case_of].transpose(1, 0, 2))))
        self.rew.copy_(torch.from_numpy(np.ascontiguousarray(d["tape_reward"][case_of].T)))
        self.pol.copy_(torch.from_numpy(np.ascontiguousarray(d["tape_policy"][case_of].transpose(1, 0, 2))))
        self.val.copy_(torch.from_numpy(np.ascontiguousarray(d["tape_value"][case_of].T)))

    def initial(self, obs):
        self.s = 0
        return self.h0, self.p0

    def recurrent(self, engine):
        s = self.s
        self.s += 1
        return self.hid[s], self.rew[s], self.pol[s], self.val[s]


@pytest.mark.parametrize("use_graph", [True, False])
def test_batched_search_tiles_the_fixture_with_changing_root_players(use_graph):
    cfg, data = gu.load("players/ckpt421_p2_sims50")
    C, B = data["seed"].shape[0], 4096
    A = data["root_policy"].shape[-1]
    m = _pkg("mcts").BatchedMCTS(B, **_hyper(cfg), use_graph=use_graph)
    heads = _TapeHeads(data, B)
    obs = torch.zeros(B, 4, device="cuda:0")
    rng = np.random.RandomState(0)
    for rep in range(3):
        case_of = rng.randint(0, C, B) if rep else np.arange(B) % C
        heads.load(case_of)
        m.seed(data["seed"][case_of].astype(np.uint64))
        to_play = data["root_to_play"][case_of].astype(np.int32)
        eng = m.run(obs, heads, train=True, to_play=torch.from_numpy(to_play).cuda() if rep == 1 else to_play)
        visits, priors, rv, _ = eng.root_stats()
        torch.cuda.synchronize()
        assert np.array_equal(visits.cpu().numpy(), data["root_visits"][case_of]), rep
        assert np.array_equal(priors.cpu().numpy(), data["root_priors"][case_of]), rep
        assert np.array_equal(rv.cpu().numpy(), data["root_value"][case_of]), rep
        n = data["tree_visit"].shape[1]
        for t in range(0, B, 61):
            d, c = eng.dump_tree(t), case_of[t]
            for f in ("visit", "value_sum", "reward", "child_base", "action"):
                assert np.array_equal(d[f][:n], data["tree_" + f][c]), (rep, t, f)
            assert np.array_equal(d["minmax"], data["minmax"][c])
        assert m._single is None and eng.last_kernel() == ""
    assert (m._graph is not None) == use_graph


# ---- (d) a cycle of alike players is the single-player search -----------------------------------------------------------------
@pytest.mark.parametrize("B,rng_mode", [(4096, "mt19937"), (20480, "philox")])
def test_alike_players_search_as_one_player(B, rng_mode):
    mcts = _pkg("mcts")
    model = _pkg("model").Muzero.from_arrays(os.path.join(gu.GOLDEN, "weights_ckpt421.npz"))
    obs = torch.from_numpy(np.random.RandomState(1).uniform(-0.05, 0.05, (B, 4)).astype(np.float32)).cuda()
    kw = dict(num_simulations=30, discount=0.999, root_exploration_fraction=0.1, rng_mode=rng_mode)
    outs = []
    for cyc in (dict(number_of_player=1, single_launch=False), dict(custom_loop="1>1")):
        m = mcts.BatchedMCTS(B, **kw, **cyc)
        m.seed(np.arange(B, dtype=np.uint64))
        heads = model.heads("cuda:0")
        to_play = dict(to_play=np.arange(B) % 2) if "custom_loop" in cyc else {}
        eng = m.run(obs, heads, train=True, **to_play)
        res = [t.cpu().numpy().copy() for t in eng.root_stats()] + [t.cpu().numpy().copy() for t in eng.act(1.0)]
        torch.cuda.synchronize()
        trees = [eng.dump_tree(t) for t in (0, 1, B // 2 + 3, B - 1)]
        assert eng.last_kernel() == "" and m._single is None
        if "custom_loop" in cyc:
            assert eng.n_cycle == 2
        outs.append((res, trees))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert np.array_equal(a, b)
    for ta, tb in zip(outs[0][1], outs[1][1]):
        for f in ("visit", "value_sum", "reward", "child_base", "action", "minmax"):
            assert np.array_equal(ta[f], tb[f]), f


# ---- (f) batched self-play: the root player is the env's move number ---------------------------------------------------------
def test_play_games_hands_the_move_number_as_root_player():
    envs_mod, sp, mcts = _pkg("envs"), _pkg("selfplay"), _pkg("mcts")
    B, T, limit = 64, 8, 3
    env = envs_mod.CartPoleVec(B, "cuda:0", seed=4, on_end="reset", limit=limit)
    env.reset()
    m = mcts.BatchedMCTS(B, num_simulations=8, discount=0.999, root_exploration_fraction=0.1, number_of_player=2)
    m.seed(np.arange(B, dtype=np.uint64))
    seen = []
    run = m.run

    def spy(*args, **kw):
        seen.append(kw["to_play"].clone())
        eng = run(*args, **kw)
        seen[-1] = (seen[-1], eng.root_player.clone())
        return eng

    m.run = spy
    chunk = sp.TrajectoryChunk(T, B, 4, 2, "cuda:0")
    sp.play_games(env, _pkg("model").Muzero.from_arrays(os.path.join(gu.GOLDEN, "weights_ckpt421.npz")).heads("cuda:0"),
                  m, 1.0, T, chunk=chunk)
    torch.cuda.synchronize()
    assert len(seen) == T
    for t, (given, staged) in enumerate(seen):
        assert (given.cpu().numpy() == t % limit).all(), t                # restarts after `limit` moves
        assert torch.equal(given.to(torch.int32), staged)
    assert (env.episode.cpu().numpy() >= 2).all()

    class NoCounter:
        obs = env.obs
    with pytest.raises(RuntimeError, match="step_count"):
        sp._search_phase(NoCounter(), None, m, chunk, 0, 1.0)


# ---- (g) the two reanalyse routes agree with two players -----------------------------------------------------------------------
def test_reanalyse_routes_agree_with_two_players():
    """reanalyse_replay_games (GameRecords) == reanalyse_replay_records (ArrayGameRecords) on the same stored games with two
    players (root player = position index), and both differ from the one-player search."""
    envs_mod, sp, mcts = _pkg("envs"), _pkg("selfplay"), _pkg("mcts")
    model = _pkg("model").Muzero.from_arrays(os.path.join(gu.GOLDEN, "weights_ckpt421.npz"))
    B, T, limit = 48, 20, 9
    env = envs_mod.CartPoleVec(B, "cuda:0", seed=3, on_end="reset", limit=limit)
    env.reset()
    m = mcts.BatchedMCTS(B, num_simulations=6, discount=0.999, root_exploration_fraction=0.1, use_graph=False)
    m.seed(np.arange(B, dtype=np.uint64))
    chunk = sp.play_games(env, model.heads("cuda:0"), m, 1.0, T)
    torch.cuda.synchronize()
    kw = dict(limit_of_game_play=limit, after_end="new_game", keep_partial=False)
    lists = sp.chunk_to_games(chunk.data, 4, 2, 0.999, **kw)
    arrays = sp.chunk_to_records(chunk, None, 2, 0.999, td_steps=4, **kw)

    def searcher(players):
        m = mcts.BatchedMCTS(128, num_simulations=8, discount=0.999, root_exploration_fraction=0.1, use_graph=False,
                             number_of_player=players)
        m.seed(np.arange(128, dtype=np.uint64))
        return m

    a = sp.reanalyse_replay_games(lists, model, searcher(2), "cuda:0", temperature=1.0, train=True)
    b = sp.reanalyse_replay_records(arrays, model, searcher(2), "cuda:0", temperature=1.0, train=True, td_steps=4)
    one = sp.reanalyse_replay_games(lists, model, searcher(1), "cuda:0", temperature=1.0, train=True)
    assert len(a) == len(b) == len(one) > 0
    assert all(isinstance(g, sp.ArrayGameRecord) for g in b)
    differs = 0
    for ga, gb, g1 in zip(a, b, one):
        assert ga.game_length == gb.game_length
        assert [int(np.argmax(x)) for x in ga.action_history] == [int(np.argmax(x)) for x in gb.action_history]
        assert np.array_equal(np.array(ga.policies), np.array(gb.policies))
        assert np.array_equal(np.array(ga.child_visits), np.array(gb.child_visits))
        assert np.array_equal(np.array(ga.root_values, np.float32), np.array(gb.root_values, np.float32))
        assert np.array_equal(np.array(ga.rewards, np.float64), np.array(gb.rewards, np.float64))
        differs += not np.array_equal(np.array(ga.child_visits), np.array(g1.child_visits))
    assert differs > 0                                          # two players search other trees than one
