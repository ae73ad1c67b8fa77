"""The refusals of the single-launch searches as a table: smz_search_mlp / _vision / _lstm / _mlp_wide / _mlp_players, their
`_act` forms and smz_search_mlp_act_cartpole.  Every row names an entry point, the engine and the arguments that provoke one
refusal, the error code and the exact text of smz_last_error(); where two conditions hold at once the row says which check
wins.  Every row is an argument check that returns before any launch: the engine's last_kernel() stays "" throughout, and one
ordinary search on the same engine succeeds after the whole table.  4 trees, 2 simulations, the smallest nets of the search
tests (test_gpu_lstm_search.py, test_gpu_mlp_wide_search.py, test_gpu_mlp_players_search.py, test_gpu_end_to_end.py)."""
import ctypes as C
import os

import pytest
import torch

import golden_util as gu
import lstm_reference as lr
import mlp_reference as mr
from test_gpu_lstm import _model as _lstm_model
from test_gpu_mlp_players_search import _ckpt421, _lib, _pkg
from test_gpu_mlp_wide_search import _net as _wide_net

pytestmark = pytest.mark.gpu

B, SIMS = 4, 2

LARGE = "{n}: large-action handles search step-wise only"
NULLARG = "{n}: null argument"
NULLOUT = "{n}_act: null output"
MULTI = "{n}: multi-player handles search step-wise only"
ONE_PLAYER = ("smz_search_mlp_players: a one-player handle (smz_set_players with more than one cycle entry selects this kernel): "
              "use smz_search_mlp")
STATS = "smz_search_mlp_players: no instrumented variant (smz_enable_stats / SMZ_DEBUG_SKIP): use the step-wise entry points"
DESC = {"smz_search_mlp": "smz_search_mlp: descriptor does not describe an LDS-resident network",
        "smz_search_vision": "smz_search_vision: descriptor does not describe a vision_model weight buffer",
        "smz_search_lstm": "smz_search_lstm: descriptor does not describe an lstm_model weight buffer",
        "smz_search_mlp_wide": "smz_search_mlp_wide: descriptor does not describe a wide mlp_model weight buffer (smz_mlp_layout_wide)",
        "smz_search_mlp_players": "smz_search_mlp_players: descriptor does not describe an LDS-resident network"}
DIMS = {"smz_search_mlp": "smz_search_mlp: network dimensions differ from the handle's",
        "smz_search_vision": "smz_search_vision: network dimensions differ from the handle's (hidden_size must be 147)",
        "smz_search_lstm": "smz_search_lstm: network dimensions differ from the handle's",
        "smz_search_mlp_wide": "smz_search_mlp_wide: network dimensions differ from the handle's",
        "smz_search_mlp_players": "smz_search_mlp_players: network dimensions differ from the handle's"}
LIMIT = {"smz_search_vision": "smz_search_vision: outside the single-launch kernel's limits (K = 2, A <= 4, S <= 32, H <= 64): "
                              "use the step-wise entry points",
         "smz_search_lstm": "smz_search_lstm: outside the single-launch kernel's limits (2 or 4 actions): use the step-wise entry points",
         "smz_search_mlp_wide": "smz_search_mlp_wide: outside the single-launch kernel's limits (2 or 4 actions): "
                                "use the step-wise entry points"}
ALPHA = "root_dirichlet_alpha must be > 0 to draw noise (numpy raises ValueError)"
TPW = "{n}: more than 64 trees per wavefront: use the step-wise entry points"
LDS = "{n}: working set exceeds the 160 KB LDS of a CU"
CARTPOLE = "smz_search_mlp_act_cartpole"


class Family:
    """One search family: its entry point, a valid descriptor / weight buffer / input tensors for B trees, and the engines the
    rows need (created on first use, all with 4 trees and 2 simulations unless a row says otherwise)."""

    def __init__(self, name, desc, weights, inputs, A, S, limit=None, env=None):
        self.name, self.desc, self.weights, self.inputs, self.A, self.S = name, desc, weights, inputs, A, S
        self.limit = limit                     # (descriptor, weights, A, K, S) of the family's action / sample limit, or None
        self.players = name == "smz_search_mlp_players"
        self.env = env
        self.engines = {}

    def engine(self, key):
        if key not in self.engines:
            eng_mod, cyc = _pkg("engine"), _pkg("mcts").cycle_values(2, None)
            A, S, kw, players = self.A, self.S, {}, self.players
            if "large" in key:
                kw["large_actions"] = True
            if key in ("multi", "large_multi"):
                players = True
            if key == "one":
                players = False
            if key == "dims":
                S = S + 1
            if key == "alpha0":
                kw["root_dirichlet_alpha"] = 0.0
            if key == "limit":
                A, kw["maxium_action_sample"], S = self.limit[2:]
            e = eng_mod.SearchEngine(B, A, S, num_simulations=600 if key == "sims600" else SIMS, **kw)
            if players:
                e.set_players(cyc)
            self.engines[key] = e
        return self.engines[key]

    def close(self):
        for e in self.engines.values():
            e.close()


def _off_by_one(desc):
    bad = type(desc).from_buffer_copy(desc)
    bad.total_floats += 1
    return bad


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _call(lib, fam, form, eng, outs, desc="own", weights="own", inputs=None, train=0, null_out=False):
    """The raw entry point: `form` is "" (plain), "_act" or "_act_cartpole"; None for a pointer argument passes NULL."""
    h = None if eng is None else eng.h
    desc = fam.desc if desc == "own" else desc
    weights = fam.weights if weights == "own" else weights
    inputs = fam.inputs if inputs is None else inputs
    d = None if desc is None else C.byref(desc)
    act = [1.0, None] + [None if null_out else _p(t) for t in outs[:3]] + [_p(outs[3])]
    if form == "_act_cartpole":
        return lib.smz_search_mlp_act_cartpole(h, d, _p(weights), train, *act, None if null_out else C.byref(fam.env), None)
    fn = getattr(lib, fam.name + form)
    return fn(h, d, _p(weights), *[_p(t) for t in inputs], train, *(act if form else []), None)


def _rows(fam):
    """(entry-point suffix, what, engine key, arguments of _call, code name, message)."""
    n = fam.name
    forms = ["", "_act"] + (["_act_cartpole"] if fam.env is not None else [])
    bad = _off_by_one(fam.desc)
    rows = []
    for form in forms:
        # the large-action and multi-player refusals of smz_search_mlp_act / _act_cartpole carry the entry point's own name
        own = n + form if n == "smz_search_mlp" else n
        rows.append((form, "large-action handle", "large", {}, "TOO_LARGE", LARGE.format(n=own)))
        rows.append((form, "large-action handle and a null descriptor", "large", dict(desc=None), "TOO_LARGE", LARGE.format(n=own)))
        if form != "_act_cartpole":
            rows.append((form, "null handle", None, {}, "INVALID", NULLARG.format(n=n)))
            rows.append((form, "null descriptor", "plain", dict(desc=None), "INVALID", NULLARG.format(n=n)))
            for i in range(len(fam.inputs)):
                ins = list(fam.inputs)
                ins[i] = None
                rows.append((form, f"null input {i}", "plain", dict(inputs=ins), "INVALID", NULLARG.format(n=n)))
        else:
            rows.append((form, "null descriptor", "plain", dict(desc=None), "INVALID",
                         CARTPOLE + ": the built-in env has 4 observations and 2 actions"))
        rows.append((form, "null weights", "plain", dict(weights=None), "INVALID", NULLARG.format(n=n)))
        if form == "_act":
            rows.append((form, "null output", "plain", dict(null_out=True), "INVALID", NULLOUT.format(n=n)))
        if form == "_act_cartpole":
            rows.append((form, "null output", "plain", dict(null_out=True), "INVALID", CARTPOLE + ": null argument"))
        if fam.players:
            rows.append((form, "one-player handle", "one", {}, "INVALID", ONE_PLAYER))
            rows.append((form, "statistics enabled", "stats", {}, "INVALID", STATS))
        else:
            rows.append((form, "multi-player handle", "multi", {}, "INVALID", MULTI.format(n=own)))
            rows.append((form, "multi-player handle and a bad descriptor", "multi", dict(desc=bad), "INVALID", MULTI.format(n=own)))
        rows.append((form, "total_floats off by one", "plain", dict(desc=bad), "INVALID", DESC[n]))
        rows.append((form, "engine of another S", "dims", {}, "INVALID", DIMS[n]))
        if fam.limit is not None:
            rows.append((form, "the family's limit", "limit", dict(desc=fam.limit[0], weights=fam.limit[1]), "TOO_LARGE", LIMIT[n]))
        rows.append((form, "train with root_dirichlet_alpha 0", "alpha0", dict(train=1), "INVALID", ALPHA))
        if n in ("smz_search_mlp_wide", "smz_search_mlp_players"):
            rows.append((form, "tpw65", "plain", {}, "TOO_LARGE", TPW.format(n=n)))
        if fam.players:
            rows.append((form, "600 simulations", "sims600", {}, "TOO_LARGE", LDS.format(n=n)))
    # which check wins, where the order differs between the entry points
    if n == "smz_search_mlp":
        rows.append(("_act", "large-action multi-player handle and a null output", "large_multi", dict(null_out=True), "TOO_LARGE",
                     LARGE.format(n=n + "_act")))
        rows.append(("_act", "multi-player handle and a null output", "multi", dict(null_out=True), "INVALID", NULLOUT.format(n=n)))
    else:
        rows.append(("_act", "large-action handle and a null output", "large", dict(null_out=True), "INVALID", NULLOUT.format(n=n)))
    return rows


def _vision_heads(A):
    model_mod = _pkg("model")
    if A == 2:
        model = model_mod.Muzero.from_state_dicts(os.path.join(gu.GOLDEN, "visionnet_L1_seed0.npz"))
    else:
        torch.manual_seed(11)
        model = model_mod.Muzero(model_structure="vision_model", observation_space_dimensions=(98, 98, 3), action_space_dimensions=A,
                                 state_space_dimensions=31, hidden_layer_dimensions=64, number_of_hidden_layer=0, random_tag=1)
        for mod in (model.representation_function, model.dynamics_function, model.afterstate_dynamics_function,
                    model.prediction_function, model.afterstate_prediction_function):
            mod.eval()
    heads = model.heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipVisionHeads" and heads.A == A
    return heads


def _family(which):
    obs = (torch.rand(B, 4, generator=torch.Generator().manual_seed(3)) - 0.5).mul(0.1).cuda().contiguous()
    if which in ("mlp", "mlp_players"):
        _, heads = _ckpt421()
        env = None
        if which == "mlp":
            state = torch.zeros(B, 4, dtype=torch.float64, device="cuda")
            env = _lib().CartPoleEnv(state.data_ptr(), obs.data_ptr(), None, None, None, None, 0, 0)
            env._keep = state
        return Family("smz_search_" + which, heads.desc, heads.weights, (obs,), heads.A, heads.S, env=env)
    if which == "vision":
        heads, three = _vision_heads(2), _vision_heads(3)
        frames = torch.rand(B, 3, 98, 98, generator=torch.Generator().manual_seed(2)).cuda()
        return Family("smz_search_vision", heads.desc, heads.weights, tuple(t.clone() for t in heads.initial(frames)), heads.A,
                      heads.S, limit=(three.desc, three.weights, 3, 3, three.S))          # three children per expansion
    if which == "lstm":
        heads = _lstm_model("lstmnet_cartpole_L1").heads("cuda:0", backend="hip")
        three = lr.fresh_net(4, 3, 16, 1, seed=3, gain=2).heads("cuda:0", backend="hip")
        assert type(heads).__name__ == type(three).__name__ == "HipLstmHeads"
        return Family("smz_search_lstm", heads.desc, heads.weights, tuple(t.clone() for t in heads.initial(obs)), heads.A, heads.S,
                      limit=(three.desc, three.weights, 3, 2, three.S))                   # three actions
    assert which == "mlp_wide"
    _, heads = _wide_net("s33")
    three = mr.fresh_net(4, 3, 33, 64, 0, seed=2).heads("cuda:0")
    assert type(three).__name__ == "HipMlpTileHeads"
    return Family("smz_search_mlp_wide", heads.wide_desc, heads.packed, tuple(t.clone() for t in heads.initial(obs)), heads.A,
                  heads.S, limit=(three.wide_desc, three.packed, 3, 2, three.S))          # three actions


@pytest.mark.parametrize("which", ["mlp", "vision", "lstm", "mlp_wide", "mlp_players"])
def test_refusal_table(which, monkeypatch):
    mod = _lib()
    lib = mod.load()
    fam = _family(which)
    scratch = fam.engine("plain")
    outs = (scratch.action, scratch.policy, scratch.child_visits, scratch.root_value)
    rows, wrong = _rows(fam), []
    print(f"{fam.name}: {len(rows)} rows")
    for form, what, key, kw, code, text in rows:
        eng = None if key is None else fam.engine("plain" if key == "stats" else key)
        if key == "stats":
            eng.enable_stats(True)
        if what == "tpw65":                                  # the environment is read on every call
            monkeypatch.setenv("SMZ_WIDE_SEARCH_TPW", "65")
            monkeypatch.setenv("SMZ_PLAYERS_SEARCH_TPW", "65")
        rc = _call(lib, fam, form, eng, outs, **kw)
        msg = lib.smz_last_error().decode()
        if what == "tpw65":
            monkeypatch.delenv("SMZ_WIDE_SEARCH_TPW")
            monkeypatch.delenv("SMZ_PLAYERS_SEARCH_TPW")
        if key == "stats":
            eng.enable_stats(False)
        if (rc, msg) != (getattr(mod, "SMZ_ERR_" + code), text):
            wrong.append((fam.name + form, what, rc, msg))
        if eng is not None:
            assert eng.last_kernel() == "", (fam.name + form, what, eng.last_kernel())
    assert not wrong, wrong
    # the engine the table was run on still searches
    eng = fam.engine("plain")
    eng.seed(0)
    search = getattr(eng, fam.name[len("smz_"):])
    search(fam.desc, fam.weights, *fam.inputs, train=True)
    visits = eng.root_stats()[0]
    torch.cuda.synchronize()
    assert (visits.cpu().numpy().sum(1) == SIMS).all()
    assert eng.last_kernel().startswith("k_" + fam.name[len("smz_"):] + "<"), eng.last_kernel()
    fam.close()
