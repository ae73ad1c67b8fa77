"""Host-resident environments: the per-env rules of the reference's Game around env.step (game.py:96-131, 223-273) over a
SLICE of a vector env's rows, the built-in CartPole stand-ins, and the worker process of the parallel stepper.

numpy + standard library only: envs.HostVecEnv runs a HostSlice in-process (the serial adapter); with `workers=N` it starts N
child processes (host_worker.py -> worker_main) that never import torch or touch the GPU, each owning a contiguous slice of
the envs and running the SAME HostSlice code on views of one shared-memory block -- the parallel stepper is the serial one by
construction, env by env.  This replaces the Ray fan-out of the reference's self-play (self_play.py:240-256: one game per
worker process) for envs that live on the host.

Shared block (SharedBlock): one file-backed mapping (/dev/shm) holding, for all B envs of the vector env,
    action i32 [B] | reward f32 [B] | flag u8 [B] | active u8 [B] | ended u8 [B] | obs <dtype> [B][row] | rec <dtype> [B][row]
and a control page: `go` (step sequence number written by the parent), `cmd`, one `done` sequence number per worker.  The
parent registers the mapping with the HIP runtime (page-locked), so rows written by a worker are DMA'd to the GPU from where
they lie.  Hand-off is by sequence numbers in shared memory (spin, then short sleeps): a step of 4096 CartPoles is ~0.1 ms of
work per worker, less than a pipe round trip.
"""
import ctypes
import mmap
import os
import pickle
import sys
import tempfile
import time

import numpy as np


def usable_cores():
    """Cores this process can actually USE: its affinity mask, capped by the container's CPU quota (cgroup v2 cpu.max / v1
    cfs_quota_us) -- the bench box shows 256 hardware threads and grants 16 CPUs' worth of time; threads beyond the quota only
    get the others throttled."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(period)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            if q > 0:
                quota = q / int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        except (OSError, ValueError):
            pass
    if quota:
        n = max(1, min(n, int(quota + 0.5)))
    return n



# ---------------------------------------------------------------------------------------------------------------------------
# built-in stand-ins (gymnasium is not part of this build)
# ---------------------------------------------------------------------------------------------------------------------------
_RS = None


def _seeded_uniform4(seed):
    """np.random.RandomState(seed).uniform(-0.05, 0.05, size=4), value for value, from ONE reseeded generator object per process:
    constructing a RandomState costs ~130 us (it first seeds itself from the OS), reseeding one ~5 us -- with thousands of envs
    the resets of finished games were most of a step."""
    global _RS
    if _RS is None:
        _RS = np.random.RandomState(0)
    _RS.seed(seed)
    return _RS.uniform(-0.05, 0.05, size=4)


class HostCartPole:
    """One CartPole-v1 shaped game on the host behind the gym call shape (reset(seed=) -> (obs, info); step(a) -> (obs,
    reward, terminated, truncated, info)): float64 Euler physics with CartPole-v1's published constants, the arithmetic
    of smz_cartpole_step.  gymnasium is not part of this build; this class is what the host-environment path is
    exercised with, and what `muzero_cli.py` uses for a single-game run."""
    metadata = {"render_fps": 50}

    def __init__(self):
        self.state = None

    def reset(self, seed=None):
        self.state = _seeded_uniform4(seed)
        return self.state.astype(np.float32), {}

    def step(self, action):
        if action not in (0, 1):
            raise ValueError(f"illegal action {action!r}")
        x, xd, th, thd = (float(v) for v in self.state)
        force = 10.0 if action == 1 else -10.0
        ct, sn = np.cos(th), np.sin(th)
        temp = (force + 0.05 * thd * thd * sn) / 1.1
        tha = (9.8 * sn - ct * temp) / (0.5 * (4.0 / 3.0 - 0.1 * ct * ct / 1.1))
        xa = temp - 0.05 * tha * ct / 1.1
        self.state = np.array([x + 0.02 * xd, xd + 0.02 * xa, th + 0.02 * thd, thd + 0.02 * tha])
        term = bool(abs(self.state[0]) > 2.4 or abs(self.state[2]) > 12 * 2 * np.pi / 360)
        return self.state.astype(np.float32), 1.0, term, False, {}

    def close(self):
        pass

    @classmethod
    def make_batch(cls, envs):
        """The batched-slice protocol (HostSlice): one object stepping all of a slice's envs with array arithmetic."""
        return CartPoleBatch(envs)


class CartPoleBatch:
    """HostCartPole.step for a whole slice at once: the state of the slice's n envs is ONE [n][4] float64 array (every env
    object's `state` becomes a row view of it) and a step is ~40 numpy operations whatever n is, instead of n Python calls of
    ~4 us.  Operation by operation the arithmetic of HostCartPole.step (same association, same numpy cos / sin), so the
    results are identical env by env -- the per-env path is the checker (tests/test_host_envs.py).

    The protocol a HostSlice asks of an env class (`make_batch(envs)` defined ON the class itself: a subclass that overrides
    step() without its own make_batch is stepped env by env):
        reset_one(i, seed) -> observation of env i after reset(seed=seed)
        step_batch(actions int64 [n], go bool [n]) -> (obs [n][...], reward float64 [n], terminated bool [n], illegal bool [n])
            steps the envs with go[i] set; an env whose action is illegal does not move and is reported in `illegal`;
            rows of envs that did not move are unspecified."""

    def __init__(self, envs):
        self.envs = list(envs)
        self.state = np.zeros((len(self.envs), 4))
        for i, e in enumerate(self.envs):
            if e.state is not None:
                self.state[i] = e.state
            e.state = self.state[i]                           # a view: render() and friends keep seeing the env's state

    def reset_one(self, i, seed):
        self.state[i] = _seeded_uniform4(seed)
        return self.state[i].astype(np.float32)

    def step_batch(self, actions, go):
        illegal = go & (actions != 0) & (actions != 1)
        move = go & ~illegal
        idx = np.nonzero(move)[0]
        n = len(self.envs)
        obs, reward, term = np.empty((n, 4), np.float32), np.zeros(n), np.zeros(n, bool)
        if len(idx):
            s = self.state[idx]
            x, xd, th, thd = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
            force = np.where(actions[idx] == 1, 10.0, -10.0)
            ct, sn = np.cos(th), np.sin(th)
            temp = (force + 0.05 * thd * thd * sn) / 1.1
            tha = (9.8 * sn - ct * temp) / (0.5 * (4.0 / 3.0 - 0.1 * ct * ct / 1.1))
            xa = temp - 0.05 * tha * ct / 1.1
            new = np.stack([x + 0.02 * xd, xd + 0.02 * xa, th + 0.02 * thd, thd + 0.02 * tha], 1)
            self.state[idx] = new
            obs[idx] = new.astype(np.float32)
            reward[idx] = 1.0
            term[idx] = (np.abs(new[:, 0]) > 2.4) | (np.abs(new[:, 2]) > 12 * 2 * np.pi / 360)
        return obs, reward, term, illegal


class HostCartPoleRender(HostCartPole):
    """HostCartPole with a render(): an H x W x 3 uint8 picture of the cart and the pole (white background, black cart,
    brown pole, a track line) -- a stand-in for CartPole-v1's pygame renderer (400 x 600 frames), which is not part of this
    image.  Drawn with numpy slices: cheap enough to feed a thousand envs from Python."""

    def __init__(self, frame_hw=(400, 600)):
        super().__init__()
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        self._img = None

    def __getstate__(self):                                 # (sent to a worker process: the frame buffer stays behind)
        d = dict(self.__dict__)
        d["_img"] = None
        return d

    def render(self):
        """The frame buffer is reused from call to call (a fresh 720 KB array costs 0.5 ms of page faults): copy it to keep it."""
        H, W = self.H, self.W
        if self._img is None:
            self._img = np.empty((H, W, 3), np.uint8)
            dy, dx = np.meshgrid([-1, 0, 1], [-1, 0, 1], indexing="ij")
            self._dy, self._dx, self._col = dy.ravel(), dx.ravel(), np.array((202, 152, 101), np.uint8)
        img = self._img
        img[...] = 255
        x, _, th, _ = (float(v) for v in self.state)
        cy = int(H * 0.75)
        img[cy + H // 40:cy + H // 40 + 1, :, :] = 0                                       # track
        cx = int(np.clip((x / 4.8 + 0.5) * W, 0, W - 1))
        cw, ch = W // 12, H // 13
        img[max(0, cy - ch // 2):cy + ch // 2, max(0, cx - cw // 2):min(W, cx + cw // 2)] = 0
        k = np.arange(0, H // 4, 2)                                                         # pole: a run of 3x3 dots
        px, py = (cx + k * np.sin(th)).astype(np.int64), (cy - ch // 2 - k * np.cos(th)).astype(np.int64)
        ok = (px >= 1) & (px < W - 1) & (py >= 1) & (py < H - 1)
        img[(py[ok][:, None] + self._dy).ravel(), (px[ok][:, None] + self._dx).ravel()] = self._col
        return img


# ---------------------------------------------------------------------------------------------------------------------------
# 2048 on the host: the rules of csrc/smz_2048.hpp and the draws of smz_2048_step_ctl, restated (include/smz.h)
# ---------------------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def smz_mix64(z):
    """smz_mix64 (csrc/smz_common.hpp) with Python integers masked to 64 bits."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def smz_unit(seed, env, epoch, comp):
    """smz_unit (csrc/smz_common.hpp): the counter-based generator's draw in [0, 1), the same double as on the device."""
    z = smz_mix64((smz_mix64((smz_mix64((seed ^ (env * 0xD1342543DE82EF95)) & _M64) + epoch) & _M64) + comp) & _M64)
    return float(z >> 11) * (1.0 / 9007199254740992.0)


def _spawn_2048(board, game_seed, n):
    """Spawn number n of a game into `board` (16 exponents, row-major): empty cell number floor(u0 * m), exponent 2 when
    u1 < 0.1, else 1."""
    empty = [i for i in range(16) if board[i] == 0]
    if not empty:
        return
    u0, u1 = smz_unit(game_seed, 0, n, 0), smz_unit(game_seed, 0, n, 1)
    board[empty[int(np.floor(u0 * len(empty)))]] = 2 if u1 < 0.1 else 1


# cells of line l, from the edge the tiles move towards, for actions 0 up, 1 right, 2 down, 3 left
_LINES_2048 = ([[4 * j + l for j in range(4)] for l in range(4)], [[4 * l + 3 - j for j in range(4)] for l in range(4)],
               [[4 * (3 - j) + l for j in range(4)] for l in range(4)], [[4 * l + j for j in range(4)] for l in range(4)])


def _dead_2048(board):
    """No action is legal: an empty board, or a full one without two equal neighbours."""
    b = np.asarray(board).reshape(4, 4)
    m = int((b == 0).sum())
    if 0 < m < 16:
        return False
    return m == 16 or not (bool((b[:, 1:] == b[:, :-1]).any()) or bool((b[1:] == b[:-1]).any()))


class Host2048:
    """One game of 2048 on the host behind the gym call shape: the game envs.Board2048Vec plays on the device, rule for rule and
    draw for draw.  reset(seed=) takes `seed` as the game's seed (spawn number n draws smz_unit(seed, 0, n, c)); an illegal move
    -- one that leaves the board unchanged, or an action outside 0 .. 3 -- raises ValueError and changes nothing.
    board: 16 uint8 exponents (0 empty, k the tile 2^k), row-major; observation = exponent / 16."""

    def __init__(self):
        self.board = np.zeros(16, np.uint8)
        self.spawns = 0
        self.game_seed = 0

    def _observation(self):
        return self.board.astype(np.float32) * np.float32(0.0625)

    def reset(self, seed=None):
        self.game_seed = int(seed or 0) & _M64
        b = [0] * 16
        _spawn_2048(b, self.game_seed, 0)
        _spawn_2048(b, self.game_seed, 1)
        self.board[:] = b                                   # (in place: a batch stepper may own the row)
        self.spawns = 2
        return self._observation(), {}

    def step(self, action):
        if not isinstance(action, (int, np.integer)) or not 0 <= int(action) < 4:
            raise ValueError(f"illegal action {action!r}")
        old = [int(v) for v in self.board]
        new, gain = list(old), 0
        for cells in _LINES_2048[int(action)]:
            out, free = [], False                           # free: the last tile of `out` may still merge
            for v in (old[c] for c in cells):
                if v == 0:
                    continue
                if free and out[-1] == v:
                    out[-1] = v + 1
                    gain += 1 << (v + 1)
                    free = False
                else:
                    out.append(v)
                    free = True
            for c, v in zip(cells, out + [0] * (4 - len(out))):
                new[c] = v
        if new == old:
            raise ValueError(f"illegal move {action!r}: the board does not change")
        _spawn_2048(new, self.game_seed, self.spawns)
        self.spawns += 1
        self.board[:] = new
        return self._observation(), float(gain), _dead_2048(new), False, {}

    def close(self):
        pass

    @classmethod
    def make_batch(cls, envs):
        return Board2048Batch(envs)


def _mix64_array(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _unit_array(seed, epoch, comp):
    """smz_unit(seed[i], 0, epoch[i], comp) for uint64 arrays (numpy's uint64 arithmetic wraps like the C one)."""
    z = _mix64_array(_mix64_array(_mix64_array(seed) + epoch) + np.uint64(comp))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _slide_lines_2048(lines):
    """Host2048.step's line rule for an array of lines [m][4] (index 0 = the edge): (new lines, gain per line)."""
    order = np.argsort(lines == 0, axis=1, kind="stable")                # tiles to the front, in order
    v = np.take_along_axis(lines, order, 1).astype(np.int64)
    a, b, c, d = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    m1 = (a == b) & (a != 0)
    m1b = m1 & (c == d) & (c != 0)                                       # the second merge behind a first one
    m2 = ~m1 & (b == c) & (b != 0)
    m3 = ~m1 & ~m2 & (c == d) & (c != 0)
    out = np.stack([np.where(m1, a + 1, a),
                    np.where(m1, np.where(m1b, c + 1, c), np.where(m2, b + 1, b)),
                    np.where(m1, np.where(m1b, 0, d), np.where(m2, d, np.where(m3, c + 1, c))),
                    np.where(m1 | m2 | m3, 0, d)], 1)
    gain = m1 * (1 << (a + 1)) + m1b * (1 << (c + 1)) + m2 * (1 << (b + 1)) + m3 * (1 << (c + 1))
    return out.astype(np.uint8), gain


def _as_lines_2048(grid, action):
    """View of boards [m][4][4] whose [m][l] is line l from the edge `action` moves towards."""
    g = grid.transpose(0, 2, 1) if action in (0, 2) else grid
    return g[:, :, ::-1] if action in (1, 2) else g


class Board2048Batch:
    """Host2048.step for a whole slice at once (the make_batch / reset_one / step_batch protocol of CartPoleBatch): the boards
    of the slice's n envs are ONE [n][16] uint8 array (every env object's `board` becomes a row view of it) and a step is a
    fixed number of numpy operations.  Same rules, same draws: the per-env class is the checker (tests/test_env2048.py)."""

    def __init__(self, envs):
        self.envs = list(envs)
        n = len(self.envs)
        self.board = np.zeros((n, 16), np.uint8)
        self.spawns = np.zeros(n, np.int64)
        self.game_seed = np.zeros(n, np.uint64)
        for i, e in enumerate(self.envs):
            self.board[i] = e.board
            self.spawns[i], self.game_seed[i] = e.spawns, e.game_seed
            e.board = self.board[i]                         # a view; the spawn counters of stepped games live here, in `spawns`

    def reset_one(self, i, seed):
        obs, _ = self.envs[i].reset(seed=seed)              # (writes through the row view)
        self.spawns[i], self.game_seed[i] = self.envs[i].spawns, self.envs[i].game_seed
        return obs

    def step_batch(self, actions, go):
        n = len(self.envs)
        actions = np.asarray(actions, np.int64)
        old = self.board.copy()
        new = old.copy().reshape(n, 4, 4)
        reward = np.zeros(n)
        for a in range(4):
            idx = np.nonzero(go & (actions == a))[0]
            if not len(idx):
                continue
            grid = old[idx].reshape(-1, 4, 4)
            out, gain = _slide_lines_2048(np.ascontiguousarray(_as_lines_2048(grid, a)).reshape(-1, 4))
            res = np.empty_like(grid)
            _as_lines_2048(res, a)[...] = out.reshape(-1, 4, 4)
            new[idx] = res
            reward[idx] = gain.reshape(-1, 4).sum(1)
        new = new.reshape(n, 16)
        moved = go & (new != old).any(1)
        illegal = go & ~moved
        idx = np.nonzero(moved)[0]
        if len(idx):
            b = new[idx]
            empty = b == 0
            m = empty.sum(1)
            epoch = self.spawns[idx].astype(np.uint64)
            u0, u1 = _unit_array(self.game_seed[idx], epoch, 0), _unit_array(self.game_seed[idx], epoch, 1)
            k = np.floor(u0 * m).astype(np.int64)
            cell = np.argmax(empty & (np.cumsum(empty, 1) - 1 == k[:, None]), 1)
            b[np.arange(len(idx)), cell] = np.where(u1 < 0.1, 2, 1)
            self.board[idx] = b
            self.spawns[idx] += 1
        g =self.board.reshape(n, 4, 4)
        m = (g == 0).sum((1, 2))
        pair = (g[:, :, 1:] == g[:, :, :-1]).any((1, 2)) | (g[:, 1:] == g[:, :-1]).any((1, 2))
        term = (m == 16) | ((m == 0) & ~pair)
        reward[~moved] = 0.0
        return self.board.astype(np.float32) * np.float32(0.0625), reward, term, illegal


# ---------------------------------------------------------------------------------------------------------------------------
# Connect Four on the host: the rules of csrc/smz_connect4.hpp, restated (include/smz.h)
# ---------------------------------------------------------------------------------------------------------------------------
_C4_SHIFTS = np.array([7 * c + r for r in range(6) for c in range(7)], np.uint64)       # bit of observation cell 7 * r + c
_C4_LINE_SHIFTS = (1, 7, 6, 8)                                                           # vertical, horizontal, the two diagonals


def _c4_line(b):
    """Four in a row in the discs of one colour: a Python integer, or a uint64 array (then an array of bools)."""
    hit = b & 0
    for s in _C4_LINE_SHIFTS:
        if isinstance(b, np.ndarray):
            m = b & (b >> np.uint64(s))
            hit = hit | (m & (m >> np.uint64(2 * s)))
        else:
            m = b & (b >> s)
            hit |= m & (m >> (2 * s))
    return hit != 0


def _c4_popcount(x):
    """Set bits of every word of a uint64 array (the usual pairwise sums; numpy's uint64 arithmetic wraps like the C one)."""
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((x * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.int64)


def connect4_observations(discs):
    """[n][2] uint64 positions -> [n][43] float32 observations: obs[7 * r + c] = +1 / -1 / 0 for a colour-0 disc, a colour-1 disc,
    an empty cell (r = 0 the bottom row); obs[42] = +1 when colour 0 is to move, else -1."""
    d = np.asarray(discs, np.uint64).reshape(-1, 2)
    obs = np.empty((len(d), 43), np.float32)
    one = np.uint64(1)
    obs[:, :42] = ((d[:, :1] >> _C4_SHIFTS) & one).astype(np.float32) - ((d[:, 1:] >> _C4_SHIFTS) & one).astype(np.float32)
    obs[:, 42] = np.where(_c4_popcount(d[:, 0] | d[:, 1]) & 1, -1.0, 1.0)
    return obs


class HostConnect4:
    """One game of Connect Four on the host behind the gym call shape: the game envs.Connect4Vec plays on the device, rule for
    rule.  The game is deterministic: reset(seed=) ignores the seed.  An illegal move -- a full column, an action outside
    0 .. 6, any move on a finished board -- raises ValueError and changes nothing.
    discs: 2 uint64 words, word p = the discs of colour p, bit 7 * c + r = column c, row r (r = 0 the bottom row)."""

    def __init__(self):
        self.discs = np.zeros(2, np.uint64)

    def _observation(self):
        return connect4_observations(self.discs)[0]

    def reset(self, seed=None):
        self.discs[:] = 0                                   # (in place: a batch stepper may own the row)
        return self._observation(), {}

    def step(self, action):
        if not isinstance(action, (int, np.integer)) or not 0 <= int(action) < 7:
            raise ValueError(f"illegal action {action!r}")
        d = [int(self.discs[0]), int(self.discs[1])]
        both = d[0] | d[1]
        count = bin(both).count("1")
        if _c4_line(d[0]) or _c4_line(d[1]) or count == 42:
            raise ValueError(f"illegal move {action!r}: the game is over")
        height = bin((both >> (7 * int(action))) & 0x3F).count("1")
        if height >= 6:
            raise ValueError(f"illegal move {action!r}: the column is full")
        colour = count & 1
        d[colour] |= 1 << (7 * int(action) + height)
        self.discs[colour] = d[colour]
        won = bool(_c4_line(d[colour]))
        return self._observation(), 1.0 if won else 0.0, won or count + 1 == 42, False, {}

    def close(self):
        pass

    @classmethod
    def make_batch(cls, envs):
        return Connect4Batch(envs)


class Connect4Batch:
    """HostConnect4.step for a whole slice at once (the make_batch / reset_one / step_batch protocol of CartPoleBatch): the
    positions of the slice's n envs are ONE [n][2] uint64 array (every env object's `discs` becomes a row view of it) and a step
    is a fixed number of numpy operations on uint64 arrays.  Same rules: the per-env class is the checker
    (tests/test_envconnect4.py)."""

    def __init__(self, envs):
        self.envs = list(envs)
        n = len(self.envs)
        self.discs = np.zeros((n, 2), np.uint64)
        for i, e in enumerate(self.envs):
            self.discs[i] = e.discs
            e.discs = self.discs[i]                         # a view

    def reset_one(self, i, seed):
        obs, _ = self.envs[i].reset(seed=seed)              # (writes through the row view)
        return obs

    def step_batch(self, actions, go):
        actions = np.asarray(actions, np.int64)
        d = self.discs
        both = d[:, 0] | d[:, 1]
        count = _c4_popcount(both)
        finished = _c4_line(d[:, 0]) | _c4_line(d[:, 1]) | (count == 42)
        in_range = (actions >= 0) & (actions < 7)
        column = np.where(in_range, actions, 0).astype(np.uint64) * np.uint64(7)
        height = _c4_popcount((both >> column) & np.uint64(0x3F))
        moved = np.asarray(go, bool) & in_range & ~finished & (height < 6)
        illegal = np.asarray(go, bool) & ~moved
        bit = np.where(moved, np.uint64(1) << (column + np.minimum(height, 5).astype(np.uint64)), np.uint64(0))
        second = (count & 1).astype(bool)
        mine = np.where(second, d[:, 1], d[:, 0]) | bit
        d[:, 0] = np.where(second, d[:, 0], mine)
        d[:, 1] = np.where(second, mine, d[:, 1])
        won = moved & _c4_line(mine)
        term = np.where(moved, won | (count + 1 == 42), finished)
        return connect4_observations(d), won.astype(np.float64), term, illegal


# ---------------------------------------------------------------------------------------------------------------------------
# Othello on the host: the rules of csrc/smz_othello.hpp, restated (include/smz.h)
# ---------------------------------------------------------------------------------------------------------------------------
_OTH_ALL = 0xFFFFFFFFFFFFFFFF
_OTH_INNER = 0x7E7E7E7E7E7E7E7E                              # the files b .. g: no run passes through the a- or the h-file
_OTH_DIRS = tuple((s, _OTH_ALL if abs(s) == 8 else _OTH_INNER) for s in (1, -1, 8, -8, 9, -9, 7, -7))
_OTH_START = (1 << 28 | 1 << 35, 1 << 27 | 1 << 36)          # colour 0 on (3,4) and (4,3), colour 1 on (3,3) and (4,4)
_OTH_SHIFTS = np.arange(64, dtype=np.uint64)


def _oth_shift(x, s):
    """One step in direction s (bits) of a Python integer or a uint64 array; what leaves the 64 bits is gone."""
    if isinstance(x, np.ndarray):
        return x << np.uint64(s) if s > 0 else x >> np.uint64(-s)
    return (x << s) & _OTH_ALL if s > 0 else x >> -s


def _oth_run(start, opp, s, mask):
    """The run of opponent discs next to `start` in direction s: one seed step and five fills (a run holds at most 6 discs)."""
    m = opp & (np.uint64(mask) if isinstance(opp, np.ndarray) else mask)
    t = m & _oth_shift(start, s)
    for _ in range(5):
        t = t | (m & _oth_shift(t, s))
    return t


def _oth_moves(me, opp):
    """The squares on which the colour with discs `me` may place a disc (Python integers, or uint64 arrays)."""
    moves = me & 0
    for s, mask in _OTH_DIRS:
        moves = moves | _oth_shift(_oth_run(me, opp, s, mask), s)
    return moves & ~(me | opp) & (np.uint64(_OTH_ALL) if isinstance(me, np.ndarray) else _OTH_ALL)


def _oth_flips(x, me, opp):
    """The opponent discs a disc placed on `x` (one bit; an array may hold 0: no flips) turns."""
    flips = me & 0
    for s, mask in _OTH_DIRS:
        t = _oth_run(x, opp, s, mask)
        closed = (_oth_shift(t, s) & me) != 0
        flips = flips | (np.where(closed, t, np.uint64(0)) if isinstance(me, np.ndarray) else (t if closed else 0))
    return flips


def othello_observations(discs, mover):
    """[n][2] uint64 positions and [n] colours to move -> [n][65] float32 observations: obs[8 * r + c] = +1 / -1 / 0 for a
    colour-0 disc, a colour-1 disc, an empty square; obs[64] = +1 when colour 0 is to move, else -1."""
    d = np.asarray(discs, np.uint64).reshape(-1, 2)
    obs = np.empty((len(d), 65), np.float32)
    one = np.uint64(1)
    obs[:, :64] = ((d[:, :1] >> _OTH_SHIFTS) & one).astype(np.float32) - ((d[:, 1:] >> _OTH_SHIFTS) & one).astype(np.float32)
    obs[:, 64] = np.where(np.asarray(mover).reshape(-1) != 0, -1.0, 1.0)
    return obs


class HostOthello:
    """One game of Othello on the host behind the gym call shape: the game envs.OthelloVec plays on the device, rule for rule.
    65 actions: 0 .. 63 place a disc of the mover on square 8 * r + c, 64 passes.  The game is deterministic: reset(seed=)
    ignores the seed.  An illegal move -- an occupied square, a placement that flips nothing, a pass while a placement exists,
    an action outside 0 .. 64, any move on a finished position -- raises ValueError and changes nothing.
    discs: 2 uint64 words, word p = the discs of colour p, bit 8 * r + c = row r, column c; mover: 1 int32, the colour to move."""

    def __init__(self):
        self.discs = np.zeros(2, np.uint64)
        self.mover = np.zeros(1, np.int32)
        self.reset()

    def _observation(self):
        return othello_observations(self.discs, self.mover)[0]

    def legal_moves(self, colour=None):
        """The placement squares of `colour` (default: the mover) as a 64-bit mask."""
        c = int(self.mover[0]) if colour is None else int(colour)
        return _oth_moves(int(self.discs[c]), int(self.discs[1 - c]))

    def reset(self, seed=None):
        self.discs[:] = _OTH_START                          # (in place: a batch stepper may own the rows)
        self.mover[:] = 0
        return self._observation(), {}

    def step(self, action):
        if not isinstance(action, (int, np.integer)) or not 0 <= int(action) <= 64:
            raise ValueError(f"illegal action {action!r}")
        action, c = int(action), int(self.mover[0])
        me, opp = int(self.discs[c]), int(self.discs[1 - c])
        mine = _oth_moves(me, opp)
        if not mine and not _oth_moves(opp, me):
            raise ValueError(f"illegal move {action!r}: the game is over")
        if action == 64:
            if mine:
                raise ValueError("illegal pass: a placement exists")
            self.mover[0] = 1 - c
            return self._observation(), 0.0, False, False, {}
        x = 1 << action
        if not x & mine:
            raise ValueError(f"illegal move {action!r}: " + ("the square is occupied" if x & (me | opp) else "it flips nothing"))
        f = _oth_flips(x, me, opp)
        me, opp = me | x | f, opp & ~f
        self.discs[c], self.discs[1 - c] = me, opp
        self.mover[0] = 1 - c
        over = not _oth_moves(opp, me) and not _oth_moves(me, opp)          # (the new mover's placements first: mostly some)
        a, b = bin(me).count("1"), bin(opp).count("1")
        return self._observation(), float((a > b) - (a < b)) if over else 0.0, over, False, {}

    def close(self):
        pass

    @classmethod
    def make_batch(cls, envs):
        return OthelloBatch(envs)


class OthelloBatch:
    """HostOthello.step for a whole slice at once (the make_batch / reset_one / step_batch protocol of CartPoleBatch): the
    positions of the slice's n envs are ONE [n][2] uint64 array and the movers ONE [n] int32 array (every env object's `discs`
    and `mover` become views of them) and a step is a fixed number of numpy operations on uint64 arrays.  Same rules: the
    per-env class is the checker (tests/test_envothello.py)."""

    def __init__(self, envs):
        self.envs = list(envs)
        n = len(self.envs)
        self.discs = np.zeros((n, 2), np.uint64)
        self.mover = np.zeros(n, np.int32)
        for i, e in enumerate(self.envs):
            self.discs[i], self.mover[i] = e.discs, e.mover[0]
            e.discs, e.mover = self.discs[i], self.mover[i:i + 1]                  # views

    def reset_one(self, i, seed):
        obs, _ = self.envs[i].reset(seed=seed)              # (writes through the views)
        return obs

    def step_batch(self, actions, go):
        actions, go = np.asarray(actions, np.int64), np.asarray(go, bool)
        d, zero = self.discs, np.uint64(0)
        second = self.mover != 0
        me, opp = np.where(second, d[:, 1], d[:, 0]), np.where(second, d[:, 0], d[:, 1])
        mine, theirs = _oth_moves(me, opp), _oth_moves(opp, me)
        finished = (mine | theirs) == 0
        square = (actions >= 0) & (actions < 64)
        x = np.where(square, np.uint64(1) << np.where(square, actions, 0).astype(np.uint64), zero)
        placed = go & ~finished & ((x & mine) != 0)
        passed = go & ~finished & (actions == 64) & (mine == 0)
        illegal = go & ~placed & ~passed
        x = np.where(placed, x, zero)
        f = _oth_flips(x, me, opp)
        me, opp = me | x | f, opp & ~f
        d[:, 0], d[:, 1] = np.where(second, opp, me), np.where(second, me, opp)
        self.mover[placed | passed] ^= 1
        over = placed & ((_oth_moves(me, opp) | _oth_moves(opp, me)) == 0)
        a, b = _c4_popcount(me), _c4_popcount(opp)
        reward = np.where(over, np.sign(a - b), 0).astype(np.float64)
        term = np.where(placed | passed, over, finished)
        return othello_observations(d, self.mover), reward, term, illegal


# ---------------------------------------------------------------------------------------------------------------------------
# observation adapters: what of env.reset / env.step's observation goes into the env's row
# ---------------------------------------------------------------------------------------------------------------------------
def tap_index(n_in, n_out):
    """Source indices of a bilinear resize n_in -> n_out as ATen's upsample_bilinear2d (align_corners False) and
    smz_frames.hip's src_index compute them: src = fma(scale, dst + 0.5, -0.5) in float32, clamped at 0; i0 = min(int(src),
    n_in - 1), i1 = min(i0 + 1, n_in - 1).  Returns int32 [2 * n_out]: (i0, i1) of every output index.  (scale * (dst + 0.5)
    and the subtraction are exact in float64, so rounding the float64 result once IS the float32 fma.)"""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float64) + 0.5
    src = (np.float64(scale) * dst - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return np.stack([i0, i1], 1).reshape(-1).astype(np.int32)


class VectorAdapter:
    """Flattened float32 observation vectors (game.py:145-167)."""
    dtype = np.float32

    def __init__(self, obs_dim, transform=None):
        self.row, self.transform = int(obs_dim), transform

    def observe(self, env, obs):
        obs = obs[0] if isinstance(obs, tuple) else obs
        if self.transform is not None:
            obs = self.transform(obs)
        return np.asarray(obs, dtype=np.float32).reshape(-1)


class FrameAdapter:
    """Rendered uint8 frames [H][W][3] (the reference's rgb_observation games, game.py:82-89, 105-107, 142-143).
    upload="frames": the row is the whole frame.  upload="taps": the row holds only the source pixels a bilinear resize to
    out_hw reads -- rows y0/y1 and columns x0/x1 of every output pixel, [2 out_h][2 out_w][3] (98 x 98 from 400 x 600: 115 KB
    instead of 720 KB per frame) -- and the device blends them with the full-frame kernel's own arithmetic
    (smz_frames_resize_taps_u8), so the two uploads give bit-identical observations."""
    dtype = np.uint8

    def __init__(self, frame_hw, out_hw, frame_source="render", upload="frames"):
        assert frame_source in ("render", "obs") and upload in ("frames", "taps")
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        self.out_h, self.out_w = int(out_hw[0]), int(out_hw[1])
        self.frame_source, self.upload = frame_source, upload
        self.row = 2 * self.out_h * 2 * self.out_w * 3 if upload == "taps" else self.H * self.W * 3
        self._lib = None

    def __getstate__(self):                                 # (sent to a worker process: the library handle is per process)
        d = dict(self.__dict__)
        d["_lib"] = None
        return d

    def _taps(self, frame):
        """The gather runs in libsmzhost.so (plain C, smzh_gather_taps_u8: ~12 us per 400 x 600 frame; numpy's fancy indexing
        needs 90-600 us for the same 115 KB) -- the one native piece a worker loads, and not a GPU library."""
        if self._lib is None:
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsmzhost.so")
            if not os.path.exists(path):
                raise RuntimeError(f"{path} is missing: build it with `make -C stochastic-muzero_amd/csrc host`")
            lib = ctypes.CDLL(path)
            lib.smzh_gather_taps_u8.restype = ctypes.c_int
            lib.smzh_gather_taps_u8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
            self._iy, self._ix = tap_index(self.H, self.out_h), tap_index(self.W, self.out_w)
            self._buf = np.empty(self.row, np.uint8)
            self._lib = lib
        frame = np.ascontiguousarray(frame)
        rc = self._lib.smzh_gather_taps_u8(frame.ctypes.data, self.H, self.W, self._iy.ctypes.data, self._iy.size,
                                           self._ix.ctypes.data, self._ix.size, self._buf.ctypes.data)
        assert rc == 0
        return self._buf                                    # (reused from call to call: HostSlice copies it into the env's row)

    def observe(self, env, obs):
        frame = env.render() if self.frame_source == "render" else (obs[0] if isinstance(obs, tuple) else obs)
        frame = np.asarray(frame)
        assert frame.shape == (self.H, self.W, 3), f"frame {frame.shape}, expected {(self.H, self.W, 3)}"
        frame = frame.astype(np.uint8, copy=False)          # (the reference: x.copy().astype(np.uint8), game.py:84)
        if self.upload == "taps":
            return self._taps(frame)
        return frame.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# the rules around env.step for a slice of envs
# ---------------------------------------------------------------------------------------------------------------------------
class HostSlice:
    """Envs [lo, hi) of a vector env and their rows in the (shared or private) buffers.  Per env it keeps what the reference's
    Game keeps around env.step (game.py:96-131, 223-273):
      * the first observation comes from env.reset(seed=env_seed + global env index [+ 1000003 * game number]);
      * a step that raises is an illegal move: observation unchanged, reward min(-steps so far, -limit, -1), termination
        flag unchanged (game.py:123-131);
      * flags: 1 terminated, 2 stopped by `limit` (game.py:270-271), 3 no step (switched off);
      * on_end "mask": a finished env is switched off (`active`); "reset": it is reset at once -- `obs` gets the fresh
        observation for the next search, `rec` keeps the post-step one for the record and `ended` marks the row."""

    def __init__(self, envs, lo, adapter, arrays, action_map, env_seed, limit, on_end, first_env, batch=True):
        self.envs, self.lo, self.n = list(envs), int(lo), len(envs)
        self.adapter, self.action_map = adapter, list(action_map)
        self.env_seed, self.limit, self.on_end, self.first_env = int(env_seed), int(limit), on_end, int(first_env)
        hi = self.lo + self.n
        for name in ("action", "reward", "flag", "active", "ended", "obs", "rec"):
            setattr(self, name, arrays[name][self.lo:hi])
        self.step_count = np.zeros(self.n, np.int64)
        self.episode = np.zeros(self.n, np.int64)
        self.done = np.zeros(self.n, bool)
        self.batch = self._make_batch() if batch else None

    def _make_batch(self):
        """The slice's batch stepper, when its envs offer one (CartPoleBatch documents the protocol): all envs of ONE class that
        defines make_batch itself, plain vector observations, an integer action map."""
        if not self.envs or not isinstance(self.adapter, VectorAdapter) or self.adapter.transform is not None:
            return None
        cls = type(self.envs[0])
        if any(type(e) is not cls for e in self.envs) or "make_batch" not in vars(cls):
            return None
        if not all(isinstance(a, (int, np.integer)) and not isinstance(a, bool) for a in self.action_map):
            return None
        self._amap = np.asarray(self.action_map, np.int64)
        return cls.make_batch(self.envs)

    def _reset_one(self, i):
        seed = self.env_seed + self.first_env + self.lo + i + 1000003 * int(self.episode[i])
        if self.batch is not None:
            self.obs[i] = np.asarray(self.batch.reset_one(i, seed), np.float32).reshape(-1)
        else:
            self.obs[i] = self.adapter.observe(self.envs[i], self.envs[i].reset(seed=seed))
        self.step_count[i] = 0
        self.done[i] = False

    def reset_all(self):
        self.episode[:] = 0
        for i in range(self.n):
            self._reset_one(i)
        self.active[:] = 1
        self.ended[:] = 0

    def _step_all_batch(self):
        """step_all's rules (below, env by env) as array operations around ONE batch.step_batch call."""
        n, limit = self.n, self.limit
        live = self.active.astype(bool)
        acts = self.action.astype(np.int64)
        in_map = (acts >= 0) & (acts < len(self._amap))       # (amap[acts[i]] raising IndexError is an illegal move too)
        mapped = self._amap[np.where(in_map, acts, 0)]
        seen, r, term, illegal = self.batch.step_batch(mapped, live & in_map)
        illegal = live & (illegal | ~in_map)
        moved = live & ~illegal
        count = self.step_count
        lim = float(limit) if limit > 0 else float("inf")
        if illegal.any():                                     # game.py:123-131: the observation stays, termination flag unchanged
            r = np.where(illegal, np.minimum(np.minimum(-count.astype(np.float64), -lim), -1.0), r)
            term = np.where(illegal, self.done, term)
        count[live] += 1
        f = np.where((limit > 0) & (count == limit), 2, np.where(term, 1, 0)).astype(np.uint8)
        self.done[live] = (term & (f != 2))[live]
        self.reward[:] = np.where(live, r, 0.0)
        self.flag[:] = np.where(live, f, 3)
        self.ended[:] = 0
        if moved.any():
            self.obs[moved] = np.asarray(seen, np.float32).reshape(n, -1)[moved]
        over = np.nonzero(live & (f != 0))[0]
        if len(over):
            if self.on_end == "reset":
                self.rec[over] = self.obs[over]
                self.ended[over] = 1
                self.episode[over] += 1
                for i in over.tolist():
                    self._reset_one(i)
            else:
                self.active[over] = 0

    def step_all(self):
        if self.batch is not None:
            return self._step_all_batch()
        envs, amap, observe = self.envs, self.action_map, self.adapter.observe
        acts, rew, flag, active, ended = self.action.tolist(), self.reward, self.flag, self.active, self.ended
        obs, rec, count = self.obs, self.rec, self.step_count
        limit, reset_mode = self.limit, self.on_end == "reset"
        ended[:] = 0
        live = active.tolist()
        for i in range(self.n):
            if not live[i]:
                flag[i], rew[i] = 3, 0.0
                continue
            env = envs[i]
            try:
                out = env.step(amap[acts[i]])
                seen, r, term = observe(env, out[0]), float(out[1]), bool(out[2])
            except Exception:                             # illegal move (game.py:123-131): the observation stays
                lim = limit if limit > 0 else float("inf")                       # Game's default limit_of_game_play
                seen, r, term = None, float(min(-int(count[i]), -lim, -1)), bool(self.done[i])
            c = count[i] = count[i] + 1
            f = 2 if (limit > 0 and c == limit) else (1 if term else 0)
            self.done[i] = term and f != 2
            rew[i], flag[i] = r, f
            if seen is not None:
                obs[i] = seen
            if f:
                if reset_mode:
                    rec[i] = obs[i]                       # the record keeps the post-step observation ...
                    ended[i] = 1
                    self.episode[i] += 1
                    self._reset_one(i)                    # ... and the next search starts from the fresh one
                else:
                    active[i] = 0

    def close(self):
        for e in self.envs:
            try:
                e.close()
            except Exception:
                pass


# ---------------------------------------------------------------------------------------------------------------------------
# the shared block
# ---------------------------------------------------------------------------------------------------------------------------
def build_env(e):
    """An env object as it is; a class or a zero-argument factory (the gymnasium.vector `env_fns` convention) is called."""
    return e() if isinstance(e, type) or (callable(e) and not hasattr(e, "step")) else e


CMD_STEP, CMD_RESET, CMD_EXIT = 1, 2, 3


def ctrl_bytes(workers):
    """Size of the control region in front of the arrays: whole 4 KB pages holding the GO word, the command slot and one 64-byte
    line per worker's done word (a fixed single page capped the worker count at 60 with a bare assertion)."""
    return (4 * done_word(max(1, int(workers))) + 4095) // 4096 * 4096


def block_layout(B, row, dtype, workers=1):
    """Byte offsets of the arrays of a B-env block, every array on a 4 KB boundary (rows of different workers never share a
    page with another array); the control region in front grows with the worker count."""
    item = np.dtype(dtype).itemsize
    out, off = {"ctrl": ctrl_bytes(workers)}, ctrl_bytes(workers)
    for name, nbytes in (("action", 4 * B), ("reward", 4 * B), ("flag", B), ("active", B), ("ended", B),
                         ("obs", B * row * item), ("rec", B * row * item)):
        out[name] = off
        off += (nbytes + 4095) // 4096 * 4096
    out["total"] = off
    return out


def map_arrays(buf, B, row, dtype, workers):
    lay = block_layout(B, row, dtype, workers)
    arr = dict(action=np.frombuffer(buf, np.int32, B, lay["action"]), reward=np.frombuffer(buf, np.float32, B, lay["reward"]),
               flag=np.frombuffer(buf, np.uint8, B, lay["flag"]), active=np.frombuffer(buf, np.uint8, B, lay["active"]),
               ended=np.frombuffer(buf, np.uint8, B, lay["ended"]),
               obs=np.frombuffer(buf, dtype, B * row, lay["obs"]).reshape(B, row),
               rec=np.frombuffer(buf, dtype, B * row, lay["rec"]).reshape(B, row))
    # control page: int32 word [GO] step sequence (futex, written by the parent); int64 slot [1] command; int32 words
    # [done_word(w)] sequence number worker w has finished (-1: attached, nothing done yet) -- written by worker w ONLY, and the
    # futex word the parent sleeps on while that worker is the one it is waiting for
    ctrl = np.frombuffer(buf, np.int64, lay["ctrl"] // 8, 0)
    if 4 * done_word(workers) > lay["ctrl"]:
        raise ValueError(f"control region of {lay['ctrl']} bytes cannot hold the done words of {workers} workers")
    return arr, ctrl, lay


def done_word(w):
    """int32 index (control page) of worker w's `done` word: one 64-byte line per worker (no false sharing between workers)."""
    return 64 + 16 * w


def control_words(buf, workers=1):
    return np.frombuffer(buf, np.int32, ctrl_bytes(workers) // 4, 0)


class SharedBlock:
    """A file-backed shared mapping created by the parent; the file is unlinked once every worker has attached."""

    def __init__(self, nbytes):
        d = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
        fd, self.path = tempfile.mkstemp(prefix="smz_hostenv_", dir=d)
        try:
            os.ftruncate(fd, nbytes)
            self.mm = mmap.mmap(fd, nbytes)
        finally:
            os.close(fd)
        self.nbytes = nbytes

    def unlink(self):
        if self.path:
            try:
                os.unlink(self.path)
            except OSError:
                pass
            self.path = None


# ---- blocking hand-off: futex words in the control page ------------------------------------------------------------------------
# Spinning workers are the wrong default: a container's CPU quota (cgroup cpu.max: 16 CPUs' worth on the 256-thread bench box)
# is burnt by every spinner, and throttling then stalls everybody -- measured: 16 spinning workers 1.9 ms per step, 64 workers
# 6.0 ms, 128 workers 12.4 ms.  Waiters sleep in the kernel on a 32-bit word of the shared control page instead (futex: a
# syscall only when there is something to wait for or somebody to wake) after a spin of a few microseconds.
#   word GO            (ctrl32[0]) step sequence number, written by the parent; workers wait for it to change
#   word done_word(w)  the sequence number worker w has finished: ONE writer per word (a bell word that every worker
#                      incremented was a non-atomic read-modify-write across processes and could go backwards, sending the parent
#                      into a full 10 ms time-out).  The parent sleeps on the word of the first worker that is not done yet.
# The store of a done word is a release store and the parent's read an acquire load (libsmzhost.so, smzh_store_release_i32 /
# smzh_load_acquire_i32) so that a worker's rows are visible before its done word on every architecture; without the library
# (not built) plain numpy stores are used, which is enough on x86's total store order.
import platform  # noqa: E402

# SYS_futex of this machine (None: unknown architecture -> waiters fall back to short sleeps); shared (not PRIVATE) futexes: the
# waiters are other processes
_SYS_FUTEX = {"x86_64": 202, "aarch64": 98, "arm64": 98}.get(platform.machine()) if sys.platform.startswith("linux") else None
_FUTEX_WAIT, _FUTEX_WAKE = 0, 1
_libc = None


class _Timespec(ctypes.Structure):
    _fields_ = [("tv_sec", ctypes.c_long), ("tv_nsec", ctypes.c_long)]


def _futex(addr, op, val, timeout_s=None):
    global _libc
    if _SYS_FUTEX is None:                                  # no futex here: a wait is a nap (the caller re-checks), a wake is nothing
        if op == _FUTEX_WAIT:
            time.sleep(min(timeout_s or 100e-6, 100e-6))
        return 0
    if _libc is None:
        _libc = ctypes.CDLL(None, use_errno=True)
        _libc.syscall.restype = ctypes.c_long
    ts = None
    if timeout_s is not None:
        ts = ctypes.byref(_Timespec(int(timeout_s), int((timeout_s % 1.0) * 1e9)))
    return _libc.syscall(_SYS_FUTEX, ctypes.c_void_p(addr), ctypes.c_int(op), ctypes.c_int(val), ts, None, ctypes.c_int(0))


def futex_wait_change(words, index, seen, timeout_s=0.05, spin=50):
    """Waits until words[index] != seen or the timeout has passed once (a short spin, then ONE kernel wait on the word: the
    caller re-checks and calls again -- spurious wake-ups and time-outs look the same to it)."""
    for _ in range(spin):
        if words[index] != seen:
            return
    _futex(words.ctypes.data + 4 * index, _FUTEX_WAIT, int(seen), timeout_s)


def futex_wake_all(words, index):
    _futex(words.ctypes.data + 4 * index, _FUTEX_WAKE, 0x7fffffff)


GO = 0                                                  # int32 word index into the control page (int64 slot 1 is the command)
_sync_lib = False


def _sync():
    """libsmzhost.so's release / acquire helpers, or None when the library is not there."""
    global _sync_lib
    if _sync_lib is False:
        _sync_lib = None
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsmzhost.so")
        if os.path.exists(path):
            try:
                lib = ctypes.CDLL(path)
                lib.smzh_store_release_i32.restype = None
                lib.smzh_store_release_i32.argtypes = [ctypes.c_void_p, ctypes.c_int32]
                lib.smzh_load_acquire_i32.restype = ctypes.c_int32
                lib.smzh_load_acquire_i32.argtypes = [ctypes.c_void_p]
                _sync_lib = lib
            except (OSError, AttributeError):
                _sync_lib = None
    return _sync_lib


def store_release(words, index, value):
    lib = _sync()
    if lib is None:
        words[index] = value
    else:
        lib.smzh_store_release_i32(words.ctypes.data + 4 * index, int(value))


def load_acquire(words, index):
    lib = _sync()
    return int(words[index]) if lib is None else int(lib.smzh_load_acquire_i32(words.ctypes.data + 4 * index))


def worker_main(spec_path):
    """Entry of a worker process (host_worker.py): attach the block, build the slice, serve step / reset commands."""
    with open(spec_path, "rb") as f:
        spec = pickle.load(f)
    fd = os.open(spec["block_path"], os.O_RDWR)
    try:
        mm = mmap.mmap(fd, spec["nbytes"])
    finally:
        os.close(fd)
    arr, ctrl, _ = map_arrays(mm, spec["B"], spec["row"], spec["dtype"], spec["workers"])
    envs = [build_env(e) for e in spec["envs"]]
    sl = HostSlice(envs, spec["lo"], spec["adapter"], arr, spec["action_map"], spec["env_seed"], spec["limit"], spec["on_end"],
                   spec["first_env"], batch=spec.get("batch", True))
    words = control_words(mm, spec["workers"])
    w, parent = spec["worker"], spec["parent_pid"]
    seq = 0
    mine = done_word(w)
    store_release(words, mine, -1)                         # attached (the parent waits for every worker's -1 -> then unlinks the file)
    try:
        while True:
            futex_wait_change(words, GO, seq, timeout_s=0.25, spin=spec.get("spin", 50))
            if words[GO] == seq:
                if os.getppid() != parent:                 # an orphaned worker exits instead of waiting for ever
                    break
                continue
            seq = load_acquire(words, GO)
            cmd = int(ctrl[1])
            if cmd == CMD_EXIT:
                break
            if cmd == CMD_RESET:
                sl.reset_all()
            else:
                sl.step_all()
            store_release(words, mine, seq)                # (this worker's own word: no read-modify-write shared with others)
            futex_wake_all(words, mine)
    finally:
        sl.close()
    return 0


if __name__ == "__main__":
    sys.exit(worker_main(sys.argv[1]))
