"""The device-resident 2048 environment (envs.Board2048Vec, smz_2048_step_ctl) against a plain-Python restatement of the rules
written here from include/smz.h (a per-line loop; it imports neither Board2048Batch nor the C core), bit for bit: boards,
draws, rewards, the illegal-move rule, the game bookkeeping and the trajectory record; shards; the host twin under
HostVecEnv; and a whole self-play iteration on it."""
import ctypes as C
import math
from importlib import import_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


# ---- the restatement ------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
OBS, A, F = 16, 4, 31


def ref_mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ref_unit(seed, env, epoch, comp):
    z = ref_mix64((seed ^ (env * 0xD1342543DE82EF95)) & M64)
    z = ref_mix64((z + epoch) & M64)
    z = ref_mix64((z + comp) & M64)
    return (z >> 11) / 9007199254740992.0


def ref_line(line):
    tiles = [v for v in line if v]
    out, gain, i = [], 0, 0
    while i < len(tiles):
        if i + 1 < len(tiles) and tiles[i] == tiles[i + 1]:
            out.append(tiles[i] + 1)
            gain += 2 ** (tiles[i] + 1)
            i += 2
        else:
            out.append(tiles[i])
            i += 1
    return out + [0] * (4 - len(out)), gain


def ref_cell(action, line, j):
    return (4 * j + line, 4 * line + 3 - j, 4 * (3 - j) + line, 4 * line + j)[action]


def ref_move(board, action):
    new, gain = list(board), 0
    for line in range(4):
        cells = [ref_cell(action, line, j) for j in range(4)]
        out, g = ref_line([board[c] for c in cells])
        gain += g
        for c, v in zip(cells, out):
            new[c] = v
    return new, gain


def ref_dead(board):
    return all(ref_move(board, a)[0] == list(board) for a in range(4))


def ref_spawn(board, game_seed, n):
    empty = [i for i in range(16) if board[i] == 0]
    u0, u1 = ref_unit(game_seed, 0, n, 0), ref_unit(game_seed, 0, n, 1)
    e = 2 if u1 < 0.1 else 1
    board[empty[int(math.floor(u0 * len(empty)))]] = e
    return e


def ref_reset(game_seed):
    board = [0] * 16
    ref_spawn(board, game_seed, 0)
    ref_spawn(board, game_seed, 1)
    return board


class RefVec:
    """B games with the bookkeeping of smz_2048_step_ctl, one env at a time."""

    def __init__(self, B, seed, first_env, on_end, limit):
        self.B, self.seed, self.first_env, self.on_end, self.limit = B, seed, first_env, on_end, limit
        self.episode, self.count, self.spawns, self.active = [0] * B, [0] * B, [2] * B, [1] * B
        self.board = [ref_reset(self.game_seed(e)) for e in range(B)]
        self.cover = dict(fours=0, illegal=0, terminated=0, limit_stops=0, restarts=0, off=0, minus_inf=0)

    def game_seed(self, e):
        return (self.seed + self.first_env + e + 1000003 * self.episode[e]) & M64

    def step(self, e, a):
        """-> (reward, flag, board the record shows | None for "no step")"""
        if self.on_end == "mask" and not self.active[e]:
            self.cover["off"] += 1
            return 0.0, 3, None
        board = self.board[e]
        new, gain = ref_move(board, a) if a in (0, 1, 2, 3) else (board, 0)
        if new == board:                                      # illegal: nothing moves, the counter still advances
            reward = float(min(-self.count[e], -self.limit if self.limit > 0 else -math.inf, -1))
            self.cover["illegal"] += 1
            self.cover["minus_inf"] += reward == -math.inf
        else:
            self.cover["fours"] += ref_spawn(new, self.game_seed(e), self.spawns[e]) == 2
            self.spawns[e] += 1
            self.board[e], reward = new, float(gain)
        dead = ref_dead(self.board[e])
        self.count[e] += 1
        flag = 2 if (self.limit > 0 and self.count[e] == self.limit) else (1 if dead else 0)
        shown = list(self.board[e])
        self.cover["terminated"] += flag == 1
        self.cover["limit_stops"] += flag == 2
        if flag and self.on_end == "reset":
            self.episode[e] += 1
            self.board[e], self.spawns[e], self.count[e] = ref_reset(self.game_seed(e)), 2, 0
            self.cover["restarts"] += 1
        elif flag and self.on_end == "mask":
            self.active[e] = 0
        return reward, flag, shown


def _obs_of(boards):
    return np.asarray(boards, np.float32).reshape(-1, 16) * np.float32(0.0625)


def _crafted(B):
    """Boards for the first envs: full but for one corner, sixteen different tiles none of which a spawn (2 or 4) can match --
    two of the four moves are illegal and the first legal one ends the game."""
    rows = {}
    for e in range(0, min(B, 24)):
        b = [3 + (i + e) % 16 for i in range(16)]
        b[(0, 3, 12, 15)[e % 4]] = 0
        rows[e] = b
    return rows


def _actions(T, B, seed):
    g = np.random.RandomState(seed)
    a = g.randint(0, 4, size=(T, B)).astype(np.int32)
    a[g.rand(T, B) < 0.03] = 4
    a[g.rand(T, B) < 0.02] = -1
    a[g.rand(T, B) < 0.01] = 1 << 30
    return a


def _search_outputs(B, seed):
    g = np.random.RandomState(seed)
    return (torch.from_numpy(g.rand(B, A)).to(DEV), torch.from_numpy(g.rand(B, A)).to(DEV),
            torch.from_numpy(g.randn(B).astype(np.float32)).to(DEV))


@pytest.mark.parametrize("on_end,limit", [("mask", 0), ("mask", 37), ("reset", 0), ("reset", 37)])
def test_device_env_equals_the_restatement_bit_for_bit(on_end, limit):
    envs = _pkg("envs")
    B, T, seed = 67, 56, 11                 # 67 = one full wavefront and a ragged tail: two workgroups, the second with 3 envs
    env = envs.Board2048Vec(B, DEV, seed=seed, on_end=on_end, limit=limit)
    assert (env.obs_dim, env.num_actions) == (16, 4) and not hasattr(env, "fused_step")
    env.reset()
    ref = RefVec(B, seed, 0, on_end, limit)
    torch.cuda.synchronize()
    assert env.board.cpu().numpy().tolist() == ref.board and (env.spawns.cpu().numpy() == 2).all()
    assert np.array_equal(env.obs.cpu().numpy(), _obs_of(ref.board))
    boards = env.board.cpu().numpy()
    for e, b in _crafted(B).items():
        boards[e] = b
        ref.board[e] = list(b)
    env.set_boards(boards)
    actions = _actions(T, B, 3)
    policy, visits, root_value = _search_outputs(B, 4)
    pol, vis, rv = policy.cpu().numpy(), visits.cpu().numpy(), root_value.cpu().numpy()
    chunk = torch.full((T, B, F), -5.0, dtype=torch.float64, device=DEV)
    shown_obs = _obs_of(ref.board)          # what `obs` holds: a switched-off env keeps its last observation
    fresh_after_end = 0
    for t in range(T):
        act = torch.from_numpy(actions[t]).to(DEV)
        env.step_and_record(act, chunk, t, policy, visits, root_value)
        torch.cuda.synchronize()
        want = np.zeros((B, F))
        reward, flag = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        for e in range(B):
            a = int(actions[t, e])
            reward[e], flag[e], shown = ref.step(e, a)
            if shown is None:
                want[e, OBS + 1] = 3.0
                continue
            want[e, :OBS] = _obs_of(shown)[0]
            want[e, OBS], want[e, OBS + 1] = reward[e], flag[e]
            want[e, OBS + 2:OBS + 2 + A] = pol[e]
            if 0 <= a < A:
                want[e, OBS + 2 + A + a] = 1.0
            want[e, OBS + 2 + 2 * A] = rv[e]
            want[e, OBS + 3 + 2 * A:] = vis[e]
            shown_obs[e] = _obs_of(ref.board[e])[0]          # (on "reset": the NEW game's board, not the record's)
            if flag[e] and on_end == "reset":
                fresh_after_end += int(not np.array_equal(shown_obs[e], want[e, :OBS])) and int((shown_obs[e] != 0).sum() == 2)
        assert env.board.cpu().numpy().tolist() == ref.board, t
        assert env.spawns.cpu().numpy().tolist() == ref.spawns, t
        assert np.array_equal(env.obs.cpu().numpy(), shown_obs), t
        assert np.array_equal(env.reward.cpu().numpy(), reward), t
        assert np.array_equal(env.terminated.cpu().numpy(), flag), t
        assert env.step_count.cpu().numpy().tolist() == ref.count, t
        assert env.episode.cpu().numpy().tolist() == ref.episode, t
        if on_end == "mask":
            assert env.active.cpu().numpy().tolist() == ref.active, t
        else:
            assert env.active is None
        assert np.array_equal(chunk[t].cpu().numpy(), want), t
    c = ref.cover
    assert c["fours"] >= 1 and c["illegal"] >= 1 and c["terminated"] >= 1, c
    if limit:
        assert c["limit_stops"] >= 1, c
    else:
        assert c["minus_inf"] >= 1, c
    if on_end == "reset":
        assert c["restarts"] >= 1 and max(ref.episode) >= 1, c
        # the record of a game's last step shows ITS board; `obs` shows the two tiles of the next game's initial board
        assert fresh_after_end == c["restarts"], (fresh_after_end, c)
    else:
        assert c["off"] >= 1, c


def _play(env, T, actions, outputs):
    sp = _pkg("selfplay")
    env.reset()
    chunk = sp.TrajectoryChunk(T, env.B, env.obs_dim, env.num_actions, env.device)
    for t in range(T):
        act = torch.from_numpy(np.ascontiguousarray(actions[t])).to(DEV)
        if hasattr(env, "step_begin"):                        # (host envs: what selfplay._search_phase enqueues)
            env.step_begin(act)
        sp._record_phase(env, chunk, t, (act,) + tuple(outputs))
    torch.cuda.synchronize()
    return chunk.data.cpu().numpy()


def test_a_shard_plays_the_rows_of_the_whole_run():
    envs = _pkg("envs")
    B, lo, T, seed = 67, 40, 50, 21
    actions = _actions(T, B, 5)
    out = _search_outputs(B, 6)
    whole_env = envs.Board2048Vec(B, DEV, seed=seed, on_end="reset", limit=37)
    whole = _play(whole_env, T, actions, out)
    part_env = envs.Board2048Vec(B - lo, DEV, seed=seed, first_env=lo, total_envs=B, on_end="reset", limit=37)
    part = _play(part_env, T, actions[:, lo:], tuple(x[lo:].contiguous() for x in out))
    assert np.array_equal(part, whole[:, lo:])
    assert torch.equal(part_env.board, whole_env.board[lo:]) and torch.equal(part_env.spawns, whole_env.spawns[lo:])
    assert torch.equal(part_env.episode, whole_env.episode[lo:]) and int(whole_env.episode.min()) >= 1


@pytest.mark.parametrize("on_end", ["mask", "reset"])
def test_host_twin_plays_the_same_games(on_end):
    """HostVecEnv over host_envs.Host2048 (stepped by Board2048Batch) and Board2048Vec: same seed, same actions, same records."""
    envs = _pkg("envs")
    B, T, seed, limit = 67, 45, 9, 37 if on_end == "reset" else 0
    actions = _actions(T, B, 8)
    out = _search_outputs(B, 2)
    dev_env = envs.Board2048Vec(B, DEV, seed=seed, on_end=on_end, limit=limit)
    host_env = envs.HostVecEnv([envs.Host2048] * B, 16, 4, DEV, env_seed=seed, limit=limit, on_end=on_end)
    try:
        assert isinstance(host_env._slice.batch, envs.Board2048Batch)
        host = _play(host_env, T, actions, out)
    finally:
        host_env.close()
    dev = _play(dev_env, T, actions, out)
    assert np.array_equal(host, dev)
    flags = dev[..., OBS + 1]
    assert (dev[..., OBS] < 0).any()                          # illegal moves on both sides
    assert (flags == 2).any() if on_end == "reset" else np.isneginf(dev[..., OBS]).any()


def test_self_play_iteration_on_the_2048_env():
    """64 envs x 130 steps, games cut at 60 moves: every returned game replays exactly through Host2048 from its game seed and its
    recorded actions; the value targets are smz_traj_targets_games' ; the search ran in one launch (k_search_mlp<4, ...>)."""
    envs, sp, he, game_mod = _pkg("envs"), _pkg("selfplay"), _pkg("host_envs"), _pkg("game")
    B, T, limit, seed, sims, td = 64, 130, 60, 13, 10, 5
    torch.manual_seed(0)
    model = _pkg("model").Muzero(model_structure="mlp_model", observation_space_dimensions=16, action_space_dimensions=4,
                                 state_space_dimensions=9, hidden_layer_dimensions=16, number_of_hidden_layer=1, random_tag=1)
    mcts = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, discount=0.997, root_exploration_fraction=0.1)
    mcts.seed(np.arange(B, dtype=np.uint64))
    env = envs.Board2048Vec(B, DEV, seed=seed, on_end="reset", limit=limit)
    games, mean_reward = sp.self_play_iteration(env, model, mcts, 1.0, T, td_steps=td)
    torch.cuda.synchronize()
    assert mcts._single is True and mcts.engine.last_kernel().startswith("k_search_mlp<4,")
    assert len(games) >= 2 * B and math.isfinite(mean_reward)
    src = games[0]._src
    chunk = torch.from_numpy(np.ascontiguousarray(src.rec.transpose(1, 0, 2))).to(DEV)
    _, target, _ = sp.chunk_targets(chunk, 16, 4, 0.997, td, after_end="new_game")
    target = target.cpu().numpy()
    nth = {}
    for g in games:
        e, t0, n = g._e, g._t0, g.game_length
        k = nth[e] = nth.get(e, -1) + 1                       # the env's k-th game of the chunk is its episode k
        twin = he.Host2048()
        obs, _ = twin.reset(seed=seed + e + 1000003 * k)
        assert n <= limit
        for i in range(n):
            onehot = np.asarray(g.action_history[i])
            assert onehot.sum() == 1.0
            a = int(onehot.argmax())
            try:
                obs, r, term = twin.step(a)[:3]
            except ValueError:                                # illegal move: nothing moves, the reference's penalty
                r, term = float(min(-i, -limit, -1)), False
            assert np.array_equal(g.observations[i].numpy().reshape(-1), obs), (e, k, i)
            assert g.rewards[i] == r, (e, k, i)
            assert term == (i == n - 1 and n < limit), (e, k, i)          # flag 0 inside a game; 1 or 2 on its last row
            assert g.make_target(i, 1, td)[0][0] == target[t0 + i, e]
            assert np.float64(game_mod.GameRecord.make_target(g, i, 1, td)[0][0]) == target[t0 + i, e]
        assert g.done == (n < limit)
    assert len(nth) == B


def test_refusals_come_back_without_a_launch():
    envs, lib_mod = _pkg("envs"), _pkg("_lib")
    lib = lib_mod.load()
    B, T = 8, 2
    env = envs.Board2048Vec(B, DEV, seed=1, on_end="reset", limit=5)
    env.reset()
    torch.cuda.synchronize()
    before = env.board.clone()
    act = torch.zeros(B, dtype=torch.int32, device=DEV)
    pol, vis, rv = _search_outputs(B, 0)
    traj = torch.zeros(T, B, F, dtype=torch.float64, device=DEV)
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def ctl(step_count=env.step_count, episode=env.episode, active=None, on_end=2):
        Q = lambda x: None if x is None else x.data_ptr()
        return lib_mod.EpisodeCtl(Q(step_count), Q(episode), Q(active), 5, on_end, 1, 0)

    def call(board=env.board, spawns=env.spawns, action=act, c=None, null_ctl=False, traj_=None, t=0, policy=pol, visits=vis,
             root=rv, n=B):
        c = ctl() if c is None else c
        return lib.smz_2048_step_ctl(P(board), P(spawns), P(action), P(env.obs), P(env.reward), P(env.terminated),
                                     None if null_ctl else C.byref(c), P(traj_), T, t, P(policy), P(visits), P(root), n, None)
    bad = lib_mod.SMZ_ERR_INVALID
    assert call(board=None) == bad and call(spawns=None) == bad and call(action=None) == bad
    assert call(null_ctl=True) == bad and call(c=ctl(step_count=None)) == bad
    assert call(n=0) == bad and call(n=-3) == bad
    assert call(c=ctl(on_end=1, active=None)) == bad and b"active_dev" in lib.smz_last_error()
    assert call(c=ctl(on_end=2, episode=None)) == bad and call(c=ctl(on_end=3)) == bad
    assert call(traj_=traj, t=T) == bad and call(traj_=traj, t=-1) == bad and b"trajectory" in lib.smz_last_error()
    assert call(traj_=traj, policy=None) == bad and call(traj_=traj, visits=None) == bad and call(traj_=traj, root=None) == bad
    assert lib.smz_2048_reset(None, P(env.spawns), P(env.obs), 1, 0, None, B, None) == bad
    assert lib.smz_2048_reset(P(env.board), None, P(env.obs), 1, 0, None, B, None) == bad
    assert lib.smz_2048_reset(P(env.board), P(env.spawns), P(env.obs), 1, 0, None, 0, None) == bad
    torch.cuda.synchronize()
    assert torch.equal(env.board, before) and int(env.step_count.sum()) == 0 and float(traj.abs().sum()) == 0.0
    assert call(traj_=traj, t=1) == 0                        # and the accepted call steps
    torch.cuda.synchronize()
    assert int(env.step_count.sum()) == B and float(traj[1].abs().sum()) > 0.0 and float(traj[0].abs().sum()) == 0.0
