"""The device-resident Connect Four environment (envs.Connect4Vec, smz_connect4_step_ctl) against a plain-Python restatement of
the rules written here from include/smz.h (a 6 x 7 list of cells and a scan of all 69 lines of four, no bitboards; it imports
neither Connect4Batch nor the C core), bit for bit: positions, observations, rewards, the illegal-move rule, the game
bookkeeping and the trajectory record; shards; the host twin under HostVecEnv; two-player self-play on it, step-wise and in
the multi-player single launch."""
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
ROWS, COLS, OBS, A, F = 6, 7, 43, 7, 67
LINES = [[(r + i * dr, c + i * dc) for i in range(4)]
         for dr, dc in ((0, 1), (1, 0), (1, 1), (-1, 1)) for r in range(ROWS) for c in range(COLS)
         if 0 <= r + 3 * dr < ROWS and 0 <= c + 3 * dc < COLS]
assert len(LINES) == 69


def ref_empty():
    return [[None] * COLS for _ in range(ROWS)]         # cells[r][c], r = 0 the bottom row; None | 0 | 1


def ref_count(cells):
    return sum(v is not None for row in cells for v in row)


def ref_has_line(cells, colour):
    return any(all(cells[r][c] == colour for r, c in line) for line in LINES)


def ref_finished(cells):
    return ref_has_line(cells, 0) or ref_has_line(cells, 1) or ref_count(cells) == ROWS * COLS


def ref_height(cells, c):
    return sum(cells[r][c] is not None for r in range(ROWS))


def ref_step(cells, action):
    """-> (cells, reward, terminated, illegal); an illegal move returns the cells it was given."""
    if action not in range(COLS) or ref_finished(cells) or ref_height(cells, action) == ROWS:
        return cells, 0.0, ref_finished(cells), True
    colour = ref_count(cells) % 2
    new = [list(row) for row in cells]
    new[ref_height(cells, action)][action] = colour
    won = ref_has_line(new, colour)
    return new, 1.0 if won else 0.0, won or ref_count(new) == ROWS * COLS, False


def ref_obs(cells):
    obs = [0.0 if cells[r][c] is None else (1.0, -1.0)[cells[r][c]] for r in range(ROWS) for c in range(COLS)]
    return np.array(obs + [1.0 if ref_count(cells) % 2 == 0 else -1.0], np.float32)


def words(cells):
    d = [0, 0]
    for r in range(ROWS):
        for c in range(COLS):
            if cells[r][c] is not None:
                d[cells[r][c]] |= 1 << (7 * c + r)
    return d


def played(moves):
    cells = ref_empty()
    for a in moves:
        cells, _, term, illegal = ref_step(cells, a)
        assert not term and not illegal
    return cells


def draw_position():
    """A full board without a line, less one top disc of the colour that is to move with 41 discs on the board (colour 1)."""
    cells = [[(r // 2 + c) & 1 for c in range(COLS)] for r in range(ROWS)]
    assert not ref_has_line(cells, 0) and not ref_has_line(cells, 1) and cells[5][1] == 1
    cells[5][1] = None
    return cells, 1


class RefVec:
    """B games with the bookkeeping of smz_connect4_step_ctl, one env at a time."""

    def __init__(self, B, on_end, limit):
        self.B, self.on_end, self.limit = B, on_end, limit
        self.cells = [ref_empty() for _ in range(B)]
        self.episode, self.count, self.active = [0] * B, [0] * B, [1] * B
        self.cover = dict(wins=[0, 0], full_column=0, out_of_range=0, draws=0, limit_stops=0, restarts=0, off=0, minus_inf=0)

    def step(self, e, a):
        """-> (reward, flag, cells the record shows | None for "no step")"""
        if self.on_end == "mask" and not self.active[e]:
            self.cover["off"] += 1
            return 0.0, 3, None
        cells = self.cells[e]
        mover = ref_count(cells) % 2
        new, reward, term, illegal = ref_step(cells, a)
        if illegal:                                           # nothing moves, the counter still advances
            reward = float(min(-self.count[e], -self.limit if self.limit > 0 else -math.inf, -1))
            self.cover["minus_inf"] += reward == -math.inf
            self.cover["out_of_range"] += a not in range(COLS)
            self.cover["full_column"] += a in range(COLS) and not term and ref_height(cells, a) == ROWS
        else:
            self.cover["wins"][mover] += reward == 1.0
            self.cover["draws"] += term and reward == 0.0
        self.cells[e] = new
        self.count[e] += 1
        flag = 2 if (self.limit > 0 and self.count[e] == self.limit) else (1 if term else 0)
        self.cover["limit_stops"] += flag == 2
        if flag and self.on_end == "reset":
            self.episode[e] += 1
            self.cells[e], self.count[e] = ref_empty(), 0
            self.cover["restarts"] += 1
        elif flag and self.on_end == "mask":
            self.active[e] = 0
        return reward, flag, new


def _crafted():
    """Positions for the first envs and the action each gets at the first step: a win by colour 0, a win by colour 1, a full
    column, the draw, and two actions out of range on the empty board."""
    draw, column = draw_position()
    return [(played([0, 1, 0, 1, 0, 1]), 0), (played([6, 0, 1, 0, 1, 0, 2]), 0), (played([3] * 6), 3), (draw, column),
            (ref_empty(), 7), (ref_empty(), -1)]


def _actions(T, B, seed):
    """Skewed towards three columns (so that columns fill up), a few out of range."""
    g = np.random.RandomState(seed)
    a = g.choice(7, size=(T, B), p=[0.04, 0.08, 0.30, 0.26, 0.24, 0.04, 0.04]).astype(np.int32)
    a[g.rand(T, B) < 0.03] = 7
    a[g.rand(T, B) < 0.02] = -1
    a[g.rand(T, B) < 0.01] = 1 << 30
    return a


def _search_outputs(B, seed):
    g = np.random.RandomState(seed)
    return (torch.from_numpy(g.rand(B, A)).to(DEV), torch.from_numpy(g.rand(B, A)).to(DEV),
            torch.from_numpy(g.randn(B).astype(np.float32)).to(DEV))


def _discs(env):
    return env.discs.cpu().numpy().view(np.uint64).tolist()


@pytest.mark.parametrize("on_end,limit", [("mask", 0), ("mask", 9), ("reset", 0), ("reset", 9)])
def test_device_env_equals_the_restatement_bit_for_bit(on_end, limit):
    envs = _pkg("envs")
    B, T = 67, 60                           # 67 = one full wavefront and a ragged tail: two workgroups, the second with 3 envs
    actions = _actions(T, B, 3)
    crafted = _crafted()
    for e, (_, a) in enumerate(crafted):
        actions[0, e] = a
    pol, vis, rv = (x.cpu().numpy() for x in _search_outputs(B, 4))
    # the restatement's whole run first: what every step must show, and what the run must contain
    ref = RefVec(B, on_end, limit)
    for e, (cells, _) in enumerate(crafted):
        ref.cells[e] = cells
    start = [words(c) for c in ref.cells]
    steps, want = [], np.zeros((T, B, F))
    for t in range(T):
        reward, flag = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        for e in range(B):
            a = int(actions[t, e])
            reward[e], flag[e], shown = ref.step(e, a)
            w = want[t, e]
            if shown is None:
                w[OBS + 1] = 3.0
                continue
            w[:OBS] = ref_obs(shown)
            w[OBS], w[OBS + 1] = reward[e], flag[e]
            w[OBS + 2:OBS + 2 + A] = pol[e]
            if 0 <= a < A:
                w[OBS + 2 + A + a] = 1.0
            w[OBS + 2 + 2 * A] = rv[e]
            w[OBS + 3 + 2 * A:] = vis[e]
        steps.append(dict(discs=[words(c) for c in ref.cells], obs=np.stack([ref_obs(c) for c in ref.cells]), reward=reward,
                          flag=flag, count=list(ref.count), episode=list(ref.episode), active=list(ref.active)))
    c = ref.cover
    assert c["wins"][0] >= 1 and c["wins"][1] >= 1 and c["full_column"] >= 1 and c["out_of_range"] >= 1 and c["draws"] >= 1, c
    if limit:
        assert c["limit_stops"] >= 1, c
    else:
        assert c["minus_inf"] >= 1, c
    if on_end == "reset":
        assert c["restarts"] >= 1 and max(ref.episode) >= 1, c
    else:
        assert c["off"] >= 1 and (want[1:, 0, OBS + 1] == 3.0).all(), c      # env 0 won at the first step: flag 3 ever after
    # the device
    env = envs.Connect4Vec(B, DEV, seed=11, on_end=on_end, limit=limit)
    assert (env.obs_dim, env.num_actions) == (43, 7) and not hasattr(env, "fused_step")
    env.reset()
    torch.cuda.synchronize()
    assert _discs(env) == [[0, 0]] * B
    assert np.array_equal(env.obs.cpu().numpy(), np.stack([ref_obs(ref_empty())] * B))
    env.set_boards(np.array(start, np.uint64))
    policy, visits, root_value = _search_outputs(B, 4)
    chunk = torch.full((T, B, F), -5.0, dtype=torch.float64, device=DEV)
    for t in range(T):
        env.step_and_record(torch.from_numpy(actions[t]).to(DEV), chunk, t, policy, visits, root_value)
        torch.cuda.synchronize()
        s = steps[t]
        assert _discs(env) == s["discs"], t
        assert np.array_equal(env.obs.cpu().numpy(), s["obs"]), t
        assert np.array_equal(env.reward.cpu().numpy(), s["reward"]), t
        assert np.array_equal(env.terminated.cpu().numpy(), s["flag"]), t
        assert env.step_count.cpu().numpy().tolist() == s["count"], t
        assert env.episode.cpu().numpy().tolist() == s["episode"], t
        if on_end == "mask":
            assert env.active.cpu().numpy().tolist() == s["active"], t
        else:
            assert env.active is None
    assert np.array_equal(chunk.cpu().numpy(), want)


def test_the_draw_on_the_device():
    envs = _pkg("envs")
    cells, column = draw_position()
    B = 3
    env = envs.Connect4Vec(B, DEV, on_end="mask")
    env.reset()
    env.set_boards(np.array([words(cells)] * B, np.uint64))
    torch.cuda.synchronize()
    assert np.array_equal(env.obs.cpu().numpy(), np.stack([ref_obs(cells)] * B))
    env.step(torch.tensor([column, 0, column], dtype=torch.int32, device=DEV))       # env 1: a full column
    torch.cuda.synchronize()
    full, reward, term, illegal = ref_step(cells, column)
    assert (reward, term, illegal) == (0.0, True, False) and ref_count(full) == 42
    assert env.terminated.cpu().tolist() == [1, 0, 1] and env.reward.cpu().tolist() == [0.0, -math.inf, 0.0]
    assert _discs(env) == [words(full), words(cells), words(full)] and env.active.cpu().tolist() == [0, 1, 0]
    assert np.array_equal(env.obs.cpu().numpy(), np.stack([ref_obs(full), ref_obs(cells), ref_obs(full)]))


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


_SHARED = {}


def _device_run(on_end):
    """Connect4Vec's record of the run the shard and the host twins are compared with, played once."""
    if on_end not in _SHARED:
        B, T, limit = 67, 45, 12 if on_end == "reset" else 0
        actions, out = _actions(T, B, 8), _search_outputs(B, 2)
        env = _pkg("envs").Connect4Vec(B, DEV, seed=9, on_end=on_end, limit=limit)
        _SHARED[on_end] = (B, T, limit, actions, out, env, _play(env, T, actions, out))
    return _SHARED[on_end]


def test_a_shard_plays_the_rows_of_the_whole_run():
    envs = _pkg("envs")
    B, T, limit, actions, out, whole_env, whole = _device_run("reset")
    lo = 40
    part_env = envs.Connect4Vec(B - lo, DEV, seed=9, first_env=lo, total_envs=B, on_end="reset", limit=limit)
    part = _play(part_env, T, actions[:, lo:], tuple(x[lo:].contiguous() for x in out))
    assert np.array_equal(part, whole[:, lo:])
    assert torch.equal(part_env.discs, whole_env.discs[lo:]) and torch.equal(part_env.step_count, whole_env.step_count[lo:])
    assert torch.equal(part_env.episode, whole_env.episode[lo:]) and int(whole_env.episode.min()) >= 1


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("on_end", ["mask", "reset"])
def test_host_twin_plays_the_same_games(on_end, workers):
    """HostVecEnv over host_envs.HostConnect4 (stepped by Connect4Batch) and Connect4Vec: same actions, same records."""
    envs = _pkg("envs")
    B, T, limit, actions, out, _, dev = _device_run(on_end)
    host_env = envs.HostVecEnv([envs.HostConnect4] * B, 43, 7, DEV, env_seed=9, limit=limit, on_end=on_end, workers=workers)
    try:
        if not workers:
            assert isinstance(host_env._slice.batch, envs.Connect4Batch)
        host = _play(host_env, T, actions, out)
    finally:
        host_env.close()
    flags = dev[..., OBS + 1]
    assert np.array_equal(host[..., OBS + 1], flags)
    # A switched-off env takes no step: smz_connect4_step_ctl leaves its record zero but for the flag 3, smz_traj_pack (the host
    # env's packer) repeats the env's last observation and the search outputs under the same flag.  Every row of a game is equal.
    stepped = flags != 3
    assert np.array_equal(host[stepped], dev[stepped]) and np.array_equal(host[..., OBS][~stepped], dev[..., OBS][~stepped])
    assert stepped.all() or on_end == "mask"
    assert (dev[..., OBS] < 0).any() and (dev[..., OBS] == 1.0).any() and (flags == 1).any()      # illegal moves, wins
    assert (flags == 2).any() if on_end == "reset" else (np.isneginf(dev[..., OBS]).any() and (flags == 3).any())


def test_two_player_self_play_end_to_end():
    """BatchedMCTS(number_of_player=2) on Connect4Vec, step-wise and in the multi-player single launch: identical chunks; the
    recorded actions replayed through HostConnect4 reproduce every recorded observation, reward and flag."""
    envs, sp, he = _pkg("envs"), _pkg("selfplay"), _pkg("host_envs")
    B, T, limit, sims = 64, 24, 14, 8
    torch.manual_seed(0)
    model = _pkg("model").Muzero(model_structure="mlp_model", observation_space_dimensions=43, action_space_dimensions=7,
                                 state_space_dimensions=9, hidden_layer_dimensions=16, number_of_hidden_layer=1, random_tag=1)
    heads = model.heads(DEV)
    assert type(heads).__name__ == "HipMlpHeads"
    chunks = []
    for flag in (False, True):
        env = envs.Connect4Vec(B, DEV, seed=13, on_end="reset", limit=limit)
        env.reset()
        m = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, use_graph=False, discount=0.997, root_exploration_fraction=0.1,
                                     number_of_player=2, players_single_launch=flag)
        m.seed(np.arange(B, dtype=np.uint64))
        chunk = sp.play_games(env, heads, m, 1.0, T)
        torch.cuda.synchronize()
        if flag:
            assert m._single is True and m.engine.last_kernel().startswith("k_search_mlp_players<"), m.engine.last_kernel()
        else:
            assert m._single is None and m.engine.last_kernel() == ""
        chunks.append(chunk.data.cpu().numpy())
        m.engine.close()
    assert np.array_equal(chunks[0], chunks[1])
    rec = chunks[0]
    assert (rec[..., OBS + 1] != 0).any()                     # at least one game ends inside the chunk
    for e in range(B):
        twin, count = he.HostConnect4(), 0
        obs, _ = twin.reset(seed=e)
        for t in range(T):
            onehot = rec[t, e, OBS + 2 + A:OBS + 2 + 2 * A]
            assert onehot.sum() == 1.0
            try:
                obs, r, term = twin.step(int(onehot.argmax()))[:3]
            except ValueError:                                # illegal move: nothing moves, the reference's penalty
                r, term = float(min(-count, -limit, -1)), False
            count += 1
            flag = 2 if count == limit else (1 if term else 0)
            assert np.array_equal(rec[t, e, :OBS], obs), (e, t)
            assert rec[t, e, OBS] == r and rec[t, e, OBS + 1] == flag, (e, t)
            if flag:
                obs, _ = twin.reset()
                count = 0


def test_refusals_come_back_without_a_launch():
    envs, lib_mod = _pkg("envs"), _pkg("_lib")
    lib = lib_mod.load()
    B, T = 8, 2
    env = envs.Connect4Vec(B, DEV, seed=1, on_end="reset", limit=5)
    env.reset()
    torch.cuda.synchronize()
    act = torch.zeros(B, dtype=torch.int32, device=DEV)
    pol, vis, rv = _search_outputs(B, 0)
    traj = torch.zeros(T, B, F, dtype=torch.float64, device=DEV)
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def ctl(step_count=env.step_count, episode=env.episode, active=None, on_end=2):
        Q = lambda x: None if x is None else x.data_ptr()
        return lib_mod.EpisodeCtl(Q(step_count), Q(episode), Q(active), 5, on_end, 1, 0)

    def call(discs=P(env.discs), action=act, c=None, null_ctl=False, traj_=None, t=0, policy=pol, visits=vis, root=rv, n=B):
        c = ctl() if c is None else c
        return lib.smz_connect4_step_ctl(discs, P(action), P(env.obs), P(env.reward), P(env.terminated),
                                         None if null_ctl else C.byref(c), P(traj_), T, t, P(policy), P(visits), P(root), n, None)
    bad = lib_mod.SMZ_ERR_INVALID
    assert call(discs=None) == bad and call(action=None) == bad
    assert call(null_ctl=True) == bad and call(c=ctl(step_count=None)) == bad
    assert call(n=0) == bad and call(n=-3) == bad
    assert call(c=ctl(on_end=1, active=None)) == bad and b"active_dev" in lib.smz_last_error()
    assert call(c=ctl(on_end=2, episode=None)) == bad and call(c=ctl(on_end=3)) == bad
    assert call(traj_=traj, t=T) == bad and call(traj_=traj, t=-1) == bad and b"trajectory" in lib.smz_last_error()
    assert call(traj_=traj, policy=None) == bad and call(traj_=traj, visits=None) == bad and call(traj_=traj, root=None) == bad
    assert call(discs=C.c_void_p(env.discs.data_ptr() + 8)) == bad and b"aligned" in lib.smz_last_error()
    assert lib.smz_connect4_reset(None, P(env.obs), B, None) == bad
    assert lib.smz_connect4_reset(P(env.discs), P(env.obs), 0, None) == bad
    assert lib.smz_connect4_reset(C.c_void_p(env.discs.data_ptr() + 8), P(env.obs), B, None) == bad
    torch.cuda.synchronize()
    assert int(env.discs.abs().sum()) == 0 and int(env.step_count.sum()) == 0 and float(traj.abs().sum()) == 0.0
    assert call(traj_=traj, t=1) == 0                        # and the accepted call steps
    torch.cuda.synchronize()
    assert int(env.step_count.sum()) == B and float(traj[1].abs().sum()) > 0.0 and float(traj[0].abs().sum()) == 0.0
    assert _discs(env) == [[1, 0]] * B                        # colour 0, column 0, bottom row


def test_the_cli_names_the_env():
    import muzero_cli
    envs = _pkg("envs")
    for name in ("Connect4", "ConnectFour-v0"):
        env = muzero_cli.make_env(name, 4, DEV, 0, limit=42, on_end="reset")
        assert isinstance(env, envs.Connect4Vec) and (env.B, env.limit, env.on_end) == (4, 42, "reset")
