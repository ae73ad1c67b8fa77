"""Which kernel path BatchedMCTS.run takes, stated as a table and checked without a GPU.

The heads are the real evaluators, built on the CPU device from the golden nets (packing needs no GPU).  The engine is a
recorder: BatchedMCTS._ensure_engine hands it out, its search_* methods log the call and, on request, refuse it with
SMZ_ERR_TOO_LARGE; _run_stepwise logs; heads.initial returns two fixed tensors of the right shape.  Every case asserts the
method called, its positional arguments by identity, the warnings and BatchedMCTS._single.

The rules (BatchedMCTS.run):
  gate          single_launch and _single is not False and num_trees <= single_launch_max_trees, for every single launch
  multi-player  only HipMlpHeads with players_single_launch: search_mlp_players(desc, weights, observations), the root players
                staged before it, no call of heads.initial; everything else step-wise, silently
  A > 32        only HipMlpLargeHeads with large_single_launch: search_mlp_large(large_desc, packed, hidden, policy)
  A <= 32       HipMlpHeads: search_mlp(desc, weights, observations); HipVisionHeads: search_vision(desc, weights, hidden,
                policy); HipLstmHeads with lstm_single_launch: search_lstm(...); HipMlpTileHeads with wide_single_launch:
                search_mlp_wide(wide_desc, packed, hidden, policy); HipMlpLargeHeads and the torch heads: step-wise
"""
import functools
import os
import warnings
from importlib import import_module

import pytest
import torch

import golden_util as gu
import mlp_reference as mr


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


FLAGS = ("lstm_single_launch", "wide_single_launch", "players_single_launch", "large_single_launch")
ALL_ON = {f: True for f in FLAGS}
TWO = dict(number_of_player=2)


@functools.lru_cache(maxsize=None)
def _heads(family):
    """One evaluator per family on the CPU device, built once (the tests replace `initial` on the instance and put it back)."""
    model_mod = _pkg("model")
    arrays = lambda f: model_mod.Muzero.from_arrays(os.path.join(gu.GOLDEN, f))
    dicts = lambda f: model_mod.Muzero.from_state_dicts(os.path.join(gu.GOLDEN, f))
    heads, cls = {
        "mlp": lambda: (arrays("weights_ckpt421.npz").heads("cpu"), "HipMlpHeads"),
        "vision": lambda: (dicts("visionnet_L1_seed0.npz").heads("cpu"), "HipVisionHeads"),
        "lstm": lambda: (dicts(os.path.join("lstm", "lstmnet_cartpole_L1.npz")).heads("cpu", backend="hip"), "HipLstmHeads"),
        "wide": lambda: (arrays("weights_ckpt450.npz").heads("cpu"), "HipMlpTileHeads"),
        "large": lambda: (mr.fresh_net(4, 40, 8, 16, 0).heads("cpu", backend="large"), "HipMlpLargeHeads"),
        "large_a4": lambda: (mr.fresh_net(4, 4, 8, 16, 0).heads("cpu", backend="large"), "HipMlpLargeHeads"),
        "torch": lambda: (arrays("weights_ckpt421.npz").heads("cpu", backend="torch"), "FusedMlpHeads"),
        "torch_a40": lambda: (mr.fresh_net(4, 40, 8, 16, 0).heads("cpu", backend="torch"), "FusedMlpHeads"),
    }[family]()
    assert type(heads).__name__ == cls
    return heads


# the six single launches: heads family, the flag that opts in (None: on by default), SearchEngine method, what the kernel takes
# ("obs": the observations, "root": the outputs of heads.initial), the names of the descriptor and the image on the heads, and the
# words of its warning (None: the LDS text of search_mlp)
LAUNCHES = {
    "mlp": ("mlp", None, "search_mlp", "obs", "desc", "weights", None),
    "vision": ("vision", None, "search_vision", "root", "desc", "weights", "vision search"),
    "lstm": ("lstm", "lstm_single_launch", "search_lstm", "root", "desc", "weights", "lstm search"),
    "wide": ("wide", "wide_single_launch", "search_mlp_wide", "root", "wide_desc", "packed", "wide mlp search"),
    "large": ("large", "large_single_launch", "search_mlp_large", "root", "large_desc", "packed", "large-action search"),
    "players": ("mlp", "players_single_launch", "search_mlp_players", "obs", "desc", "weights", "multi-player search"),
}
REFUSAL = "outside this kernel's limits"


class _Engine:
    """Stands in for SearchEngine: logs what BatchedMCTS calls on it."""

    def __init__(self, log):
        self.log, self.refuse, self.code = log, False, _pkg("_lib").SMZ_ERR_TOO_LARGE

    def set_root_player(self, to_play):
        self.log.append(("set_root_player", to_play))

    def __getattr__(self, name):
        if not name.startswith("search_"):
            raise AttributeError(name)

        def search(*args, **kw):
            self.log.append((name, args, kw))
            if self.refuse:
                raise _pkg("_lib").SmzError(self.code, REFUSAL)
        return search


class _Harness:
    def __init__(self, monkeypatch, family, num_trees=8, **mcts_kw):
        self.heads = _heads(family)
        self.log = []
        self.eng = _Engine(self.log)
        self.m = m = _pkg("mcts").BatchedMCTS(num_trees, num_simulations=5, **mcts_kw)
        self.obs = torch.zeros(4, 3)
        self.hidden, self.policy = torch.zeros(4, self.heads.S), torch.zeros(4, self.heads.A)

        def ensure(num_actions, hidden_size):
            self.log.append(("engine", num_actions, hidden_size))
            return self.eng

        def stepwise(observations, heads, train):
            self.log.append(("stepwise", observations, heads, train))
            return self.eng

        def initial(obs, **kw):
            self.log.append(("initial", obs, kw))
            return self.hidden, self.policy

        m._ensure_engine, m._run_stepwise = ensure, stepwise
        monkeypatch.setattr(self.heads, "initial", initial, raising=False)

    def run(self, **kw):
        """One run(): (the log entries it added, the texts of the warnings it gave)."""
        del self.log[:]
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            eng = self.m.run(self.obs, self.heads, **kw)
        assert eng is self.eng
        return list(self.log), [str(w.message) for w in seen]

    def expect_single(self, launch, log, train=True, act_temperature=None, env_step=None, record=None, to_play=0):
        """`log` is exactly the calls of this single launch, in order, and the search got these very objects."""
        _, _, method, takes, desc, image, _ = LAUNCHES[launch]
        h = self.heads
        A, S = int(h.A), int(h.S)
        if takes == "root":
            (name, obs, kw), log = log[0], log[1:]
            assert name == "initial" and obs is self.obs
            assert (set(kw) == {"record"} and kw["record"] is record) if record is not None else kw == {}
        assert log[0] == ("engine", A, S)
        if launch == "players":
            assert log[1] == ("set_root_player", to_play)
            log = log[1:]
        assert len(log) == 2, log
        name, args, kw = log[1]
        assert name == method
        want = (getattr(h, desc), getattr(h, image)) + ((self.obs,) if takes == "obs" else (self.hidden, self.policy))
        assert len(args) == len(want) and all(a is b for a, b in zip(args, want))
        assert kw.pop("train") is train and kw.pop("act_temperature") == act_temperature
        if launch == "mlp":
            assert kw.pop("env_step") is env_step
        assert kw == {}

    def expect_stepwise(self, log, train=True):
        assert len(log) == 1 and log[0][0] == "stepwise", log
        assert log[0][1] is self.obs and log[0][2] is self.heads and log[0][3] is train

    def warning(self, launch):
        what = LAUNCHES[launch][6]
        if what is None:
            return (f"single-launch search does not fit in LDS for this batch geometry ({self.m.num_trees} trees x "
                    f"{self.m.num_simulations} simulations): using the step-wise kernels")
        err = f"libsmz error {_pkg('_lib').SMZ_ERR_TOO_LARGE}: {REFUSAL}"
        return f"single-launch {what} is outside its limits for this configuration ({err}): using the step-wise kernels"


def _kw(launch):
    """The constructor arguments that let `launch` run: its opt-in flag, and two players for the multi-player one."""
    flag = LAUNCHES[launch][1]
    return dict({} if flag is None else {flag: True}, **(TWO if launch == "players" else {}))


# (heads family, BatchedMCTS arguments, the single launch expected or None for the step-wise kernels)
CASES = [
    # default flags: the two launches that need no opt-in
    ("mlp", {}, "mlp"), ("vision", {}, "vision"), ("lstm", {}, None), ("wide", {}, None), ("large", {}, None),
    ("large_a4", {}, None), ("torch", {}, None), ("torch_a40", {}, None),
    # its own opt-in on
    ("lstm", dict(lstm_single_launch=True), "lstm"), ("wide", dict(wide_single_launch=True), "wide"),
    ("large", dict(large_single_launch=True), "large"),
    # every opt-in on: each family keeps its own kernel; large heads with at most 32 actions and the torch heads have none
    ("mlp", ALL_ON, "mlp"), ("vision", ALL_ON, "vision"), ("lstm", ALL_ON, "lstm"), ("wide", ALL_ON, "wide"),
    ("large", ALL_ON, "large"), ("large_a4", ALL_ON, None), ("torch", ALL_ON, None), ("torch_a40", ALL_ON, None),
    # another family's opt-in
    ("lstm", dict(wide_single_launch=True, large_single_launch=True, players_single_launch=True), None),
    ("wide", dict(lstm_single_launch=True, large_single_launch=True, players_single_launch=True), None),
    ("large", dict(lstm_single_launch=True, wide_single_launch=True, players_single_launch=True), None),
    # single_launch=False
    ("mlp", dict(single_launch=False), None), ("vision", dict(single_launch=False), None),
    ("lstm", dict(ALL_ON, single_launch=False), None), ("wide", dict(ALL_ON, single_launch=False), None),
    ("large", dict(ALL_ON, single_launch=False), None),
    # one tree more than single_launch_max_trees, and exactly that many
    ("mlp", dict(num_trees=17409), None), ("vision", dict(num_trees=17409), None), ("lstm", dict(ALL_ON, num_trees=17409), None),
    ("wide", dict(ALL_ON, num_trees=17409), None), ("large", dict(ALL_ON, num_trees=17409), None),
    ("mlp", dict(num_trees=17408), "mlp"), ("large", dict(ALL_ON, num_trees=17408), "large"),
    # two players: only HipMlpHeads with players_single_launch
    ("mlp", TWO, None), ("vision", TWO, None), ("lstm", dict(TWO, lstm_single_launch=True), None),
    ("wide", dict(TWO, wide_single_launch=True), None), ("large", dict(TWO, large_single_launch=True), None),
    ("mlp", dict(TWO, players_single_launch=True), "players"), ("mlp", dict(ALL_ON, **TWO), "players"),
    ("mlp", dict(ALL_ON, custom_loop="1>2>1>3"), "players"),
    ("vision", dict(ALL_ON, **TWO), None), ("lstm", dict(ALL_ON, **TWO), None), ("wide", dict(ALL_ON, **TWO), None),
    ("large", dict(ALL_ON, **TWO), None), ("large_a4", dict(ALL_ON, **TWO), None), ("torch", dict(ALL_ON, **TWO), None),
    ("mlp", dict(ALL_ON, single_launch=False, **TWO), None), ("mlp", dict(ALL_ON, num_trees=17409, **TWO), None),
    # one player: players_single_launch alone changes nothing
    ("mlp", dict(players_single_launch=True), "mlp"), ("lstm", dict(players_single_launch=True), None),
]


def _case_id(c):
    return c[0] + "-" + ("default" if not c[1] else ",".join(f"{k}={v}" for k, v in sorted(c[1].items()))) + "->" + str(c[2])


def test_single_launch_max_trees_is_17408():
    assert _pkg("mcts").SINGLE_LAUNCH_MAX_TREES == 17408 and _pkg("mcts").BatchedMCTS(4).single_launch_max_trees == 17408
    assert _pkg("_lib").MAX_ACTIONS == 32


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("family,kw,launch", CASES, ids=[_case_id(c) for c in CASES])
def test_dispatch(monkeypatch, family, kw, launch, train):
    h = _Harness(monkeypatch, family, **kw)
    for rep in range(2):                       # the second search of an object takes the same path
        log, warned = h.run(train=train)
        assert warned == []
        if launch is None:
            h.expect_stepwise(log, train=train)
            assert h.m._single is None
        else:
            h.expect_single(launch, log, train=train)
            assert h.m._single is True
        assert h.eng.obs_recorded is False


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_act_temperature_reaches_the_single_launch(monkeypatch, launch):
    h = _Harness(monkeypatch, LAUNCHES[launch][0], **_kw(launch))
    log, warned = h.run(act_temperature=0.25)
    h.expect_single(launch, log, act_temperature=0.25)
    assert warned == []


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_a_refused_launch_warns_once_and_stays_stepwise(monkeypatch, launch):
    """SMZ_ERR_TOO_LARGE before any single launch has run: the call is made, one warning with the family's text, the step-wise
    kernels, _single False; after that no further attempt and no further warning."""
    h = _Harness(monkeypatch, LAUNCHES[launch][0], **_kw(launch))
    h.eng.refuse = True
    log, warned = h.run()
    h.expect_single(launch, log[:-1])
    h.expect_stepwise(log[-1:])
    assert warned == [h.warning(launch)] and h.m._single is False
    h.eng.refuse = False                       # (it would be taken now; it is not tried)
    for rep in range(2):
        log, warned = h.run()
        h.expect_stepwise(log)
        assert warned == [] and h.m._single is False


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_a_refusal_after_a_success_raises(monkeypatch, launch):
    h = _Harness(monkeypatch, LAUNCHES[launch][0], **_kw(launch))
    log, warned = h.run()
    h.expect_single(launch, log)
    assert h.m._single is True
    h.eng.refuse = True
    with pytest.raises(_pkg("_lib").SmzError) as err:
        h.run()
    assert err.value.code == _pkg("_lib").SMZ_ERR_TOO_LARGE and h.m._single is True
    assert [e[0] for e in h.log if e[0] == "stepwise"] == []


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_any_other_error_is_a_failure_not_a_slow_path(monkeypatch, launch):
    h = _Harness(monkeypatch, LAUNCHES[launch][0], **_kw(launch))
    h.eng.refuse, h.eng.code = True, _pkg("_lib").SMZ_ERR_HIP
    with pytest.raises(_pkg("_lib").SmzError):
        h.run()
    assert h.m._single is None and [e[0] for e in h.log if e[0] == "stepwise"] == []


def test_env_step_is_passed_only_with_an_act_temperature(monkeypatch):
    env = object()
    h = _Harness(monkeypatch, "mlp")
    log, _ = h.run(env_step=env)
    h.expect_single("mlp", log, env_step=None)
    log, _ = h.run(env_step=env, act_temperature=1.0)
    h.expect_single("mlp", log, env_step=env, act_temperature=1.0)
    log, _ = h.run(act_temperature=1.0)
    h.expect_single("mlp", log, act_temperature=1.0)
    # no other launch takes it
    for launch in ("vision", "lstm", "wide", "large", "players"):
        h = _Harness(monkeypatch, LAUNCHES[launch][0], **_kw(launch))
        log, _ = h.run(env_step=env, act_temperature=1.0)
        h.expect_single(launch, log, act_temperature=1.0)


def test_record_obs_goes_to_the_vision_root_launch(monkeypatch):
    """record= is passed to heads.initial only when given; obs_recorded says that the root launch ran with it, also when the
    search launch behind it was refused; the step-wise path (which evaluates the root itself) records nothing."""
    rec = torch.zeros(4, 3)
    h = _Harness(monkeypatch, "vision")
    log, _ = h.run()
    h.expect_single("vision", log)
    assert h.eng.obs_recorded is False
    log, _ = h.run(record_obs=rec)
    h.expect_single("vision", log, record=rec)
    assert h.eng.obs_recorded is True
    log, _ = h.run()
    assert h.eng.obs_recorded is False

    h = _Harness(monkeypatch, "vision")
    h.eng.refuse = True
    log, warned = h.run(record_obs=rec)
    h.expect_single("vision", log[:-1], record=rec)
    h.expect_stepwise(log[-1:])
    assert warned == [h.warning("vision")] and h.eng.obs_recorded is True
    log, warned = h.run(record_obs=rec)
    h.expect_stepwise(log)
    assert warned == [] and h.eng.obs_recorded is False

    for kw in (dict(single_launch=False), TWO):
        h = _Harness(monkeypatch, "vision", **kw)
        log, _ = h.run(record_obs=rec)
        h.expect_stepwise(log)
        assert h.eng.obs_recorded is False
    # heads of the other rooted launches are not handed a record
    for launch in ("lstm", "wide", "large"):
        h = _Harness(monkeypatch, LAUNCHES[launch][0], **_kw(launch))
        log, _ = h.run(record_obs=rec)
        h.expect_single(launch, log)
        assert h.eng.obs_recorded is False


def test_to_play_is_staged_before_the_multi_player_launch(monkeypatch):
    to_play = torch.zeros(8, dtype=torch.int32)
    h = _Harness(monkeypatch, "mlp", **_kw("players"))
    log, _ = h.run(to_play=to_play)
    assert log[1][0] == "set_root_player" and log[1][1] is to_play
    h.expect_single("players", log, to_play=to_play)
    log, _ = h.run()
    h.expect_single("players", log, to_play=0)
