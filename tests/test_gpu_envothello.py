"""The device-resident Othello environment (envs.OthelloVec, smz_othello_step_ctl) against the plain-Python restatement of
tests/othello_ref.py (cells and rays, no bitboards; it imports neither OthelloBatch nor the C core), bit for bit: positions,
movers, observations, rewards, the illegal-move rule, the game bookkeeping and the trajectory record; shards; the host twin
under HostVecEnv; two-player self-play on a large-action handle."""
import ctypes as C
import math
from importlib import import_module

import numpy as np
import pytest
import torch

import othello_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, A, F = R.OBS, R.A, R.F


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


class RefVec:
    """B games with the bookkeeping of smz_othello_step_ctl, one env at a time."""

    def __init__(self, B, on_end, limit):
        self.B, self.on_end, self.limit = B, on_end, limit
        self.cells, self.mover = [R.start() for _ in range(B)], [0] * B
        self.episode, self.count, self.active = [0] * B, [0] * B, [1] * B
        self.cover = dict(wins=[0, 0], passes=0, refused_pass=0, occupied=0, no_flip=0, out_of_range=0, early=0, limit_stops=0,
                          restarts=0, off=0, minus_inf=0)

    def legal(self, e):
        return R.legal_actions(self.cells[e], self.mover[e])

    def step(self, e, a):
        """-> (reward, flag, (cells, mover) the record shows | None for "no step")"""
        if self.on_end == "mask" and not self.active[e]:
            self.cover["off"] += 1
            return 0.0, 3, None
        cells, mover, c = self.cells[e], self.mover[e], self.cover
        new, mover2, reward, term, illegal = R.step(cells, mover, a)
        if illegal:                                           # nothing moves, the counter still advances
            reward = R.illegal_reward(self.count[e], self.limit)
            c["minus_inf"] += reward == -math.inf
            c["out_of_range"] += not 0 <= a <= R.PASS
            if not term:
                c["refused_pass"] += a == R.PASS
                if 0 <= a < 64:
                    occupied = cells[a // 8][a % 8] is not None
                    c["occupied"] += occupied
                    c["no_flip"] += not occupied
        else:
            c["passes"] += a == R.PASS
            if term:
                c["early"] += R.count(new) < 64
                if reward:
                    c["wins"][mover if reward > 0 else 1 - mover] += 1
        self.cells[e], self.mover[e] = new, mover2
        self.count[e] += 1
        flag = 2 if (self.limit > 0 and self.count[e] == self.limit) else (1 if term else 0)
        c["limit_stops"] += flag == 2
        if flag and self.on_end == "reset":
            self.episode[e] += 1
            self.cells[e], self.mover[e], self.count[e] = R.start(), 0, 0
            c["restarts"] += 1
        elif flag and self.on_end == "mask":
            self.active[e] = 0
        return reward, flag, (new, mover2)


def _crafted():
    """(cells, mover, first action) for the first envs: the 8-direction placement, a wipe-out by either colour, a legal pass, a
    refused pass, an action on a finished position, an occupied square, an action out of range, and the runs to the a- and
    h-files (the refused ones are placements that flip nothing)."""
    out = [R.all_directions(), R.wipe_out(0), R.wipe_out(1), R.legal_pass(), R.refused_pass(), R.finished_position() + (5,),
           (R.start(), 0, 27), (R.start(), 0, -1)]
    return out + [(cells, mover, action) for cells, mover, action, _ in R.edge_runs()]


_SCRIPT = {}


def _script(B, T):
    """Start positions and actions of a run of B envs over T steps, the same for every on_end / limit: env e starts from the
    position a restatement game reaches after k random legal moves, k spread over 0 .. 58 (the first envs: the crafted
    positions), and at every step gets a uniformly chosen legal action of the restatement's with probability 0.85, otherwise one
    uniform in -1 .. 66, a few 1 << 30.  The actions walk a restatement of their own ("reset" bookkeeping without a limit), so
    under the other settings some of the 'legal' ones are refused: the comparison does not depend on which."""
    if (B, T) in _SCRIPT:
        return _SCRIPT[(B, T)]
    g = np.random.RandomState(65)
    crafted = _crafted()
    start = []
    for e in range(B):
        if e < len(crafted):
            start.append(crafted[e][:2])
            continue
        cells, mover, k = R.start(), 0, (e * 58) // (B - 1)
        for _ in range(k):
            legal = R.legal_actions(cells, mover)
            if not legal:
                break
            cells, mover = R.step(cells, mover, legal[g.randint(len(legal))])[:2]
        start.append((cells, mover))
    walk = RefVec(B, "reset", 0)
    actions = np.zeros((T, B), np.int32)
    for e, (cells, mover) in enumerate(start):
        walk.cells[e], walk.mover[e] = cells, mover
    for t in range(T):
        for e in range(B):
            legal, u = walk.legal(e), g.rand()
            if t == 0 and e < len(crafted):
                a = crafted[e][2]
            elif u < 0.85 and legal:
                a = legal[g.randint(len(legal))]
            else:
                a = (1 << 30) if u > 0.995 else g.randint(-1, 67)
            actions[t, e] = a
            walk.step(e, int(a))
    _SCRIPT[(B, T)] = (start, actions)
    return _SCRIPT[(B, T)]


def _search_outputs(B, seed):
    g = np.random.RandomState(seed)
    return (torch.from_numpy(g.rand(B, A)).to(DEV), torch.from_numpy(g.rand(B, A)).to(DEV),
            torch.from_numpy(g.randn(B).astype(np.float32)).to(DEV))


def _discs(env):
    return env.discs.cpu().numpy().view(np.uint64).tolist()


def _set(env, start):
    env.set_boards(np.array([R.words(c) for c, _ in start], np.uint64), np.array([m for _, m in start], np.int32))


@pytest.mark.parametrize("on_end,limit", [("mask", 0), ("mask", 9), ("reset", 0), ("reset", 9)])
def test_device_env_equals_the_restatement_bit_for_bit(on_end, limit):
    envs = _pkg("envs")
    k_envs = envs.OthelloVec.envs_per_group
    B, T = 2 * k_envs + 3, 40               # two full workgroups and a ragged one
    start, actions = _script(B, T)
    pol, vis, rv = (x.cpu().numpy() for x in _search_outputs(B, 4))
    # the restatement's whole run first: what every step must show, and what the run must contain
    ref = RefVec(B, on_end, limit)
    for e, (cells, mover) in enumerate(start):
        ref.cells[e], ref.mover[e] = cells, mover
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
            w[:OBS] = R.obs(*shown)
            w[OBS], w[OBS + 1] = reward[e], flag[e]
            w[OBS + 2:OBS + 2 + A] = pol[e]
            if 0 <= a < A:
                w[OBS + 2 + A + a] = 1.0
            w[OBS + 2 + 2 * A] = rv[e]
            w[OBS + 3 + 2 * A:] = vis[e]
        steps.append(dict(discs=[R.words(c) for c in ref.cells], mover=list(ref.mover),
                          obs=np.stack([R.obs(c, m) for c, m in zip(ref.cells, ref.mover)]), reward=reward, flag=flag,
                          count=list(ref.count), episode=list(ref.episode), active=list(ref.active)))
    c = ref.cover
    print(c)
    assert c["wins"][0] >= 1 and c["wins"][1] >= 1 and c["passes"] >= 1 and c["refused_pass"] >= 1 and c["occupied"] >= 1, c
    assert c["no_flip"] >= 1 and c["out_of_range"] >= 1 and c["early"] >= 1, c
    if limit:
        assert c["limit_stops"] >= 1, c
    else:
        assert c["minus_inf"] >= 1, c
    if on_end == "reset":
        assert c["restarts"] >= 1 and max(ref.episode) >= 1, c
    else:
        assert c["off"] >= 1 and (want[1:, 0, OBS + 1] == 3.0).all(), c      # env 0's game ended at the first step: flag 3 ever after
    # the device
    env = envs.OthelloVec(B, DEV, seed=11, on_end=on_end, limit=limit)
    assert (env.obs_dim, env.num_actions, env.rec_obs_dim) == (65, 65, 65) and not hasattr(env, "fused_step")
    env.reset()
    torch.cuda.synchronize()
    assert _discs(env) == [R.words(R.start())] * B and env.mover.cpu().tolist() == [0] * B
    assert np.array_equal(env.obs.cpu().numpy(), np.stack([R.obs(R.start(), 0)] * B))
    _set(env, start)
    policy, visits, root_value = _search_outputs(B, 4)
    chunk = torch.full((T, B, F), -5.0, dtype=torch.float64, device=DEV)
    for t in range(T):
        env.step_and_record(torch.from_numpy(actions[t]).to(DEV), chunk, t, policy, visits, root_value)
        torch.cuda.synchronize()
        s = steps[t]
        assert _discs(env) == s["discs"], t
        assert env.mover.cpu().tolist() == s["mover"], t
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


def _play(env, T, actions, outputs, start=None):
    sp = _pkg("selfplay")
    env.reset()
    if start is not None:
        _set(env, start)
    chunk = sp.TrajectoryChunk(T, env.B, env.obs_dim, env.num_actions, env.device, rec_obs_dim=OBS)
    assert chunk.obs is None and chunk.F == F
    for t in range(T):
        act = torch.from_numpy(np.ascontiguousarray(actions[t])).to(DEV)
        if hasattr(env, "step_begin"):                        # (host envs: what selfplay._search_phase enqueues)
            env.step_begin(act)
        sp._record_phase(env, chunk, t, (act,) + tuple(outputs))
    torch.cuda.synchronize()
    return chunk.data.cpu().numpy()


def _start_actions(B, T, seed):
    """Actions for games from the start position (the host twin starts there): the restatement walks B games with "reset"
    bookkeeping; a legal action with probability 0.85, else one uniform in -1 .. 66."""
    g = np.random.RandomState(seed)
    walk = RefVec(B, "reset", 0)
    actions = np.zeros((T, B), np.int32)
    for t in range(T):
        for e in range(B):
            legal, u = walk.legal(e), g.rand()
            a = legal[g.randint(len(legal))] if (u < 0.85 and legal) else g.randint(-1, 67)
            actions[t, e] = a
            walk.step(e, int(a))
    return actions


_SHARED = {}


def _device_run(on_end):
    """OthelloVec's record of the run the shard and the host twins are compared with, played once."""
    if on_end not in _SHARED:
        envs = _pkg("envs")
        B, T, limit = 2 * envs.OthelloVec.envs_per_group + 3, 40, 12 if on_end == "reset" else 0
        actions, out = _start_actions(B, T, 8), _search_outputs(B, 2)
        env = envs.OthelloVec(B, DEV, seed=9, on_end=on_end, limit=limit)
        _SHARED[on_end] = (B, T, limit, actions, out, env, _play(env, T, actions, out))
    return _SHARED[on_end]


def test_a_shard_plays_the_rows_of_the_whole_run():
    """first_env = 40 of B: the same rows, from the crafted and mid-game positions of the bit-for-bit run."""
    envs = _pkg("envs")
    B, T, lo, limit = 2 * envs.OthelloVec.envs_per_group + 3, 40, 40, 9
    B = max(B, lo + 3)
    start, actions = _script(B, T)
    out = _search_outputs(B, 2)
    whole_env = envs.OthelloVec(B, DEV, seed=9, on_end="reset", limit=limit)
    whole = _play(whole_env, T, actions, out, start)
    part_env = envs.OthelloVec(B - lo, DEV, seed=9, first_env=lo, total_envs=B, on_end="reset", limit=limit)
    part = _play(part_env, T, actions[:, lo:], tuple(x[lo:].contiguous() for x in out), start[lo:])
    assert np.array_equal(part, whole[:, lo:])
    assert torch.equal(part_env.discs, whole_env.discs[lo:]) and torch.equal(part_env.mover, whole_env.mover[lo:])
    assert torch.equal(part_env.step_count, whole_env.step_count[lo:])
    assert torch.equal(part_env.episode, whole_env.episode[lo:]) and int(whole_env.episode.min()) >= 1


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("on_end", ["mask", "reset"])
def test_host_twin_plays_the_same_games(on_end, workers):
    """HostVecEnv over host_envs.HostOthello (stepped by OthelloBatch) and OthelloVec: same actions, same records."""
    envs = _pkg("envs")
    B, T, limit, actions, out, _, dev = _device_run(on_end)
    host_env = envs.HostVecEnv([envs.HostOthello] * B, OBS, A, DEV, env_seed=9, limit=limit, on_end=on_end, workers=workers)
    try:
        if not workers:
            assert isinstance(host_env._slice.batch, envs.OthelloBatch)
        host = _play(host_env, T, actions, out)
    finally:
        host_env.close()
    flags = dev[..., OBS + 1]
    assert np.array_equal(host[..., OBS + 1], flags)
    # A switched-off env takes no step: smz_othello_step_ctl leaves its record zero but for the flag 3, smz_traj_pack (the host
    # env's packer) repeats the env's last observation and the search outputs under the same flag.  Every row of a game is equal.
    stepped = flags != 3
    assert np.array_equal(host[stepped], dev[stepped]) and np.array_equal(host[..., OBS][~stepped], dev[..., OBS][~stepped])
    assert stepped.all() or on_end == "mask"
    assert (dev[..., OBS] < -1).any() and (dev[..., :64] != dev[0, 0, :64]).any()             # illegal moves, moved boards
    assert (flags == 2).any() if on_end == "reset" else np.isneginf(dev[..., OBS]).any()


def test_two_player_self_play_end_to_end():
    """BatchedMCTS(number_of_player=2) on OthelloVec, on a large-action handle with the heads Muzero.heads picks: two runs give
    identical chunks; the recorded actions replayed through HostOthello reproduce every recorded observation, reward and flag;
    the record holds legal moves."""
    envs, sp, he, lib_mod = _pkg("envs"), _pkg("selfplay"), _pkg("host_envs"), _pkg("_lib")
    B, T, limit, sims = 64, 24, 14, 8
    torch.manual_seed(0)
    model = _pkg("model").Muzero(model_structure="mlp_model", observation_space_dimensions=OBS, action_space_dimensions=A,
                                 state_space_dimensions=9, hidden_layer_dimensions=16, number_of_hidden_layer=1, random_tag=1)
    heads = model.heads(DEV)
    print("heads:", type(heads).__name__)
    chunks = []
    for _ in range(2):
        env = envs.OthelloVec(B, DEV, seed=13, on_end="reset", limit=limit)
        env.reset()
        m = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, use_graph=False, discount=0.997, root_exploration_fraction=0.1,
                                     number_of_player=2)
        m.seed(np.arange(B, dtype=np.uint64))
        chunk = sp.play_games(env, heads, m, 1.0, T)
        torch.cuda.synchronize()
        assert m.engine.large_actions and m.engine.A == A > lib_mod.MAX_ACTIONS       # a large-action handle
        assert chunk.obs is None and tuple(chunk.data.shape) == (T, B, F)
        chunks.append(chunk.data.cpu().numpy())
        m.engine.close()
    assert np.array_equal(chunks[0], chunks[1])
    rec = chunks[0]
    legal_moves = 0
    for e in range(B):
        twin, count = he.HostOthello(), 0
        obs, _ = twin.reset(seed=e)
        for t in range(T):
            onehot = rec[t, e, OBS + 2 + A:OBS + 2 + 2 * A]
            assert onehot.sum() == 1.0
            before = obs
            try:
                obs, r, term = twin.step(int(onehot.argmax()))[:3]
                legal_moves += 1
                assert r >= 0 or term
                assert not np.array_equal(obs, before)        # (a pass changes obs[64], a placement the board)
            except ValueError:                                # illegal move: nothing moves, the reference's penalty
                r, term = float(min(-count, -limit, -1)), False
            count += 1
            flag = 2 if count == limit else (1 if term else 0)
            assert np.array_equal(rec[t, e, :OBS], obs), (e, t)
            assert rec[t, e, OBS] == r and rec[t, e, OBS + 1] == flag, (e, t)
            if flag:
                obs, _ = twin.reset()
                count = 0
    print("legal moves recorded:", legal_moves, "of", T * B)
    assert (rec[..., OBS + 1] != 0).any()                     # at least one game ends inside the chunk (the limit)
    # a legal move: reward >= 0 with a changed board.  About 4 of 65 actions are legal at the start position.
    changed = (rec[1:, :, :64] != rec[:-1, :, :64]).any(-1) & (rec[1:, :, OBS] >= 0) & (rec[:-1, :, OBS + 1] == 0)
    assert legal_moves >= 1 and changed.any(), legal_moves


def test_refusals_come_back_without_a_launch():
    envs, lib_mod = _pkg("envs"), _pkg("_lib")
    lib = lib_mod.load()
    B, T = 8, 2
    env = envs.OthelloVec(B, DEV, seed=1, on_end="reset", limit=5)
    env.reset()
    torch.cuda.synchronize()
    discs0, obs0 = env.discs.clone(), env.obs.clone()
    act = torch.full((B,), 19, dtype=torch.int32, device=DEV)
    pol, vis, rv = _search_outputs(B, 0)
    traj = torch.zeros(T, B, F, dtype=torch.float64, device=DEV)
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def ctl(step_count=env.step_count, episode=env.episode, active=None, on_end=2):
        Q = lambda x: None if x is None else x.data_ptr()
        return lib_mod.EpisodeCtl(Q(step_count), Q(episode), Q(active), 5, on_end, 1, 0)

    def call(discs=P(env.discs), mover=P(env.mover), action=act, c=None, null_ctl=False, traj_=None, t=0, policy=pol, visits=vis,
             root=rv, n=B):
        c = ctl() if c is None else c
        return lib.smz_othello_step_ctl(discs, mover, P(action), P(env.obs), P(env.reward), P(env.terminated),
                                        None if null_ctl else C.byref(c), P(traj_), T, t, P(policy), P(visits), P(root), n, None)
    bad = lib_mod.SMZ_ERR_INVALID
    assert call(discs=None) == bad and call(mover=None) == bad and call(action=None) == bad
    assert call(null_ctl=True) == bad and call(c=ctl(step_count=None)) == bad
    assert call(n=0) == bad and call(n=-3) == bad
    assert call(c=ctl(on_end=1, active=None)) == bad and b"active_dev" in lib.smz_last_error()
    assert call(c=ctl(on_end=2, episode=None)) == bad and call(c=ctl(on_end=3)) == bad
    assert call(traj_=traj, t=T) == bad and call(traj_=traj, t=-1) == bad and b"trajectory" in lib.smz_last_error()
    assert call(traj_=traj, policy=None) == bad and call(traj_=traj, visits=None) == bad and call(traj_=traj, root=None) == bad
    assert call(discs=C.c_void_p(env.discs.data_ptr() + 8)) == bad and b"aligned" in lib.smz_last_error()
    assert lib.smz_othello_reset(None, P(env.mover), P(env.obs), B, None) == bad
    assert lib.smz_othello_reset(P(env.discs), None, P(env.obs), B, None) == bad
    assert lib.smz_othello_reset(P(env.discs), P(env.mover), P(env.obs), 0, None) == bad
    assert lib.smz_othello_reset(C.c_void_p(env.discs.data_ptr() + 8), P(env.mover), P(env.obs), B, None) == bad
    torch.cuda.synchronize()
    assert torch.equal(env.discs, discs0) and torch.equal(env.obs, obs0) and int(env.mover.sum()) == 0
    assert int(env.step_count.sum()) == 0 and float(traj.abs().sum()) == 0.0 and float(env.reward.abs().sum()) == 0.0
    assert call(traj_=traj, t=1) == 0                        # and the accepted call steps
    torch.cuda.synchronize()
    assert int(env.step_count.sum()) == B and float(traj[1].abs().sum()) > 0.0 and float(traj[0].abs().sum()) == 0.0
    assert _discs(env) == [R.words(R.step(R.start(), 0, 19)[0])] * B and env.mover.cpu().tolist() == [1] * B


def test_the_cli_names_the_env():
    import muzero_cli
    envs = _pkg("envs")
    for name in ("Othello", "Othello-v0", "Reversi"):
        env = muzero_cli.make_env(name, 4, DEV, 0, limit=120, on_end="reset")
        assert isinstance(env, envs.OthelloVec) and (env.B, env.limit, env.on_end) == (4, 120, "reset")
