"""The HIP root evaluation of the wide and the large-action mlp_model heads (csrc/smz_mlp_root.hip: smz_mlp_initial_wide /
smz_mlp_initial_large through heads.HipMlpTileHeads / HipMlpLargeHeads with hip_root=True, Muzero.heads(hip_root=True)),
against the float64 restatement of tests/mlp_reference.py.  Shapes are (obs, A, S, H, L).

What each shape is the first to exercise:
  wide  (1,1,1,1,0)         every dimension 1; S = 1: hidden exactly 0 on both sides
  wide  (3,2,5,7,2)         obs and S end inside an 8-input group; the mid layer applied twice
  wide  (8,3,8,8,0)         no padding input anywhere
  wide  (9,2,61,126,0)      a second obs group holding one input; the widths of config 434
  wide  (4,2,61,126,4)      checkpoint 450
  wide  (128,64,64,128,1)   the 8 KB tile filled exactly, A + S = 128
  wide  (129,2,8,16,1)      the first observation wider than the 8 KB tile
  wide  (1024,67,61,126,0)  the obs limit (a 64 KB tile, two wavefronts per workgroup) with A + S = 128
  large (4,100,29,64,0)     the smallest shape the wide layout refuses
  large (4,128,8,16,1)      one panel filled
  large (4,129,8,16,1)      the softmax across a panel boundary
  large (361,362,32,64,1)   a Go board
  large (4,1000,16,64,1)    eight panels, ragged last
  large (1024,1024,64,128,4) every limit at once

Tolerances are those of tests/test_gpu_mlp_envelope.py, taken from there: the bound of an output is max(contract, 4 x e32),
contract = TILE_ATOL (hidden rows 4e-6, policies 2e-6), e32 = the largest error of the float32 Restatement against the float64
one on the same rows, recomputed on the CPU in every run.  No row is left out: every case asserts on the CPU, before it touches
the GPU, that the float64 restatement alone has no root_span in [0.5e-5, 2e-5] (S >= 2).  The nets are mlp_reference.fresh_net
with the representation's parameters multiplied by the gain too (fresh_net leaves the representation as initialised).

Measured on MI355X (profiles/mlp_root_heads_tolerances.jsonl is one run with SMZ_TOLERANCE_LOG set), worst over all cases of this
file: hidden rows 1.5e-6 ((1024,1024,64,128,4) at gain 16; bound 4e-6), policies 4.0e-7 ((4,2,61,126,4) at gain 16; bound 2e-6),
policy row sums within 1.9e-7 of 1 (bound 1e-6).  The contract bound was the active one in every case (4 x e32 stayed below it:
e32 at most 8.3e-7 on hidden rows, 4.4e-7 on policies), no row left out.

Launch geometry, the same at every batch size.  smz_mlp_initial_wide: a wavefront per 16-row tile; four wavefronts per
workgroup while four observation tiles fit 160 KB (obs <= 640), two above -- (1024,67,61,126,0) runs the latter; at most 2048
workgroups, so with four wavefronts row 131 072 starts the second grid-stride trip of workgroup 0's first wavefront: B =
131 089 runs it, ragged at the end.  smz_mlp_initial_large: a workgroup of four wavefronts per tile, the tile's policy panels
shared among them (A <= 128: wavefronts 1 to 3 bring no maximum; A = 129, 362, 1000 / 1024: panels % 4 = 2, 3, 0); at most 2048
workgroups: row 32 768 starts the second trip of workgroup 0, B = 32 785 runs it."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

import mlp_reference as mr
from test_gpu_large_heads_search import _Recording, _Tape, _search
from test_gpu_large_actions import _streams_equal, _trees_equal
from test_gpu_lstm import _held
from test_gpu_lstm_envelope import NAN_BITS, _guarded, _untouched
from test_gpu_mlp_envelope import TILE_ATOL
from test_gpu_mlp_wide_search import _rng, _same_dumps, _same_states, _snapshot

pytestmark = pytest.mark.gpu

WIDE = [(1, 1, 1, 1, 0), (3, 2, 5, 7, 2), (8, 3, 8, 8, 0), (9, 2, 61, 126, 0), (4, 2, 61, 126, 4), (128, 64, 64, 128, 1),
        (129, 2, 8, 16, 1), (1024, 67, 61, 126, 0)]
LARGE = [(4, 100, 29, 64, 0), (4, 128, 8, 16, 1), (4, 129, 8, 16, 1), (361, 362, 32, 64, 1), (4, 1000, 16, 64, 1),
         (1024, 1024, 64, 128, 4)]
CASES = [("wide", s) for s in WIDE] + [("large", s) for s in LARGE]
GAINS = (1, 4, 16)
ROWS = 531                                  # 33 full tiles and a ragged one
EDGE_WIDE, EDGE_LARGE = (129, 2, 8, 16, 1), (4, 129, 8, 16, 1)
# the first row of the second grid-stride trip (2048 workgroups; wide: four tiles each, large: one), and a ragged last tile
SECOND_TRIP = dict(wide=2048 * 4 * 16 + 17, large=2048 * 16 + 17)
DISTINCT = 67                               # distinct rows of the geometry batches: coprime with 16, every row meets every column


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _id(case):
    return case[0] + "_" + "x".join(str(v) for v in case[1])


def _net(shape, seed, gain):
    """mlp_reference.fresh_net with the representation's parameters multiplied by the gain as well."""
    model = mr.fresh_net(*shape, seed=seed, gain=gain)
    with torch.no_grad():
        for p in model.representation_function.parameters():
            p.mul_(float(gain))
    return model


def _obs(shape, seed, rows=ROWS):
    return torch.randn(rows, shape[0], generator=torch.Generator().manual_seed(seed))


def _root_heads(layout, model, shape):
    """hip_root heads of the layout: the large ones through Muzero.heads, the wide ones built directly ("auto" hands the small
    shapes to the LDS-resident kernels) unless "auto" picks them anyway."""
    if layout == "large":
        heads = model.heads("cuda:0", backend="large", hip_root=True)
        assert type(heads).__name__ == "HipMlpLargeHeads"
    else:
        heads = model.heads("cuda:0", hip_root=True)
        if type(heads).__name__ != "HipMlpTileHeads":
            model_mod, heads_mod = _pkg("model"), _pkg("heads")
            arrays = model_mod.mlp_arrays_from_modules(model.representation_function, model.prediction_function,
                                                       model.afterstate_prediction_function, model.afterstate_dynamics_function,
                                                       model.dynamics_function)
            heads = heads_mod.HipMlpTileHeads(arrays, dict(zip(("obs", "A", "S", "H", "L"), shape)), "cuda:0", hip_root=True)
    assert heads.hip_root and "initial" in vars(heads)          # (the HIP root is bound on the instance)
    return heads


def _references(model, o, S):
    """float64 and float32 restatements of the root on rows `o`, the CPU assertion that no row sits at the + 1e-5 discontinuity
    of the scaling, e32 and the bounds."""
    root64, root32 = mr.Restatement(model).initial(o), mr.Restatement(model, torch.float32).initial(o)
    span = root64["root_span"]
    if S >= 2:
        assert not bool(((span >= 0.5e-5) & (span <= 2e-5)).any()), float(span.min())
    else:
        assert (span == 0).all()
    e32 = {k: float((root64["root_" + k] - root32["root_" + k].double()).abs().max()) for k in ("hidden", "policy")}
    return root64, e32, {k: max(TILE_ATOL[k], 4 * e32[k]) for k in e32}


def _root_matches(tag, shape, hid, pol, root64, bound):
    _, A, S, _, _ = shape
    assert hid.shape == (root64["root_hidden"].shape[0], S) and pol.shape == (hid.shape[0], A)
    if S == 1:          # span exactly 0 on both sides: (x - x) / 1e-5
        assert (hid == 0).all() and (root64["root_hidden"] == 0).all()
    _held(f"{tag} hidden", hid, root64["root_hidden"], bound["hidden"])
    _held(f"{tag} policy", pol, root64["root_policy"], bound["policy"])
    assert bool((pol >= 0).all())
    _held(f"{tag} policy row sums", pol.double().sum(1), torch.ones(pol.shape[0], dtype=torch.float64), 1e-6)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_hip_root_matches_the_float64_restatement(case, gain):
    """531 rows (33 full tiles and a ragged one) of randn observations per shape and gain, net seed 200 + i, input seed 11 + i."""
    layout, shape = case
    i = CASES.index(case)
    model = _net(shape, 200 + i, gain)
    o = _obs(shape, 11 + i)
    root64, e32, bound = _references(model, o, shape[2])
    tag = f"root {_id(case)} gain {gain}"
    print(f"{tag}: e32 " + ", ".join(f"{k} {v:.2e}" for k, v in e32.items()))
    heads = _root_heads(layout, model, shape)
    hid, pol = (t.clone().cpu() for t in heads.initial(o.cuda().contiguous()))
    _root_matches(tag, shape, hid, pol, root64, bound)


def _launch(layout, heads, o):
    """The entry point through ctypes on the test's own guarded buffers -> hidden and policy as int32 bit patterns [B, width]."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    n = o.shape[0]
    fn, desc = (lib.smz_mlp_initial_large, heads.large_desc) if layout == "large" else (lib.smz_mlp_initial_wide, heads.wide_desc)
    widths = dict(hidden=heads.S, policy=heads.A)
    out = {k: _guarded(n, w) for k, w in widths.items()}
    p = lambda t: C.c_void_p(t.data_ptr())
    od = o.cuda().contiguous()
    lib_mod.check(fn(C.byref(desc), p(heads.packed), p(od), p(out["hidden"]), p(out["policy"]), n,
                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for k, w in widths.items():
        assert _untouched(out[k], n, w), (n, k)
        assert not bool((out[k][:n * w] == NAN_BITS).any()), (n, k)
    return {k: out[k][:n * w].view(n, w).cpu() for k, w in widths.items()}


@pytest.mark.parametrize("case", [("wide", EDGE_WIDE), ("large", EDGE_LARGE)], ids=_id)
def test_rows_do_not_depend_on_the_batch_and_nothing_else_is_written(case):
    """(129,2,8,16,1) and (4,129,8,16,1), gain 4.  67 distinct observation rows, each evaluated in a batch of 1; then batches of
    1, 16, 17 (a ragged second tile; large: a second workgroup), 64 and 65 (wide: a second workgroup) and 131 089 / 32 785 rows
    (wide / large: the second grid-stride trip, ragged at the end) whose row r is distinct row r % 67: every output row is, bit for bit, the batch-of-1 result of its observation,
    the 8 guard rows behind row B - 1 of either output keep their NaN pattern and every element inside is written."""
    layout, shape = case
    model = _net(shape, 160, 4)
    heads = _root_heads(layout, model, shape)
    distinct = _obs(shape, 81, DISTINCT)
    ones = [_launch(layout, heads, distinct[i:i + 1]) for i in range(DISTINCT)]
    want = {k: torch.cat([r[k] for r in ones], 0) for k in ("hidden", "policy")}
    assert len({tuple(r) for r in want["hidden"].tolist()}) == DISTINCT
    for rows in (1, 16, 17, 64, 65, SECOND_TRIP[layout]):
        idx = torch.arange(rows) % DISTINCT
        got = _launch(layout, heads, distinct[idx])
        for k, v in got.items():
            assert torch.equal(v, want[k][idx]), (rows, k)
    root64, _, bound = _references(model, distinct, shape[2])
    _root_matches(f"root {_id(case)} batch of 1", shape, want["hidden"].view(torch.float32), want["policy"].view(torch.float32),
                  root64, bound)


def _wide_runs(heads, B, sims, rng, obs, train=True):
    """eager step-wise, graph replay and the single launch on the same heads: root statistics, act outputs, three dumped trees
    and their stream positions of each."""
    mcts_mod = _pkg("mcts")
    res = {}
    for name, kw in (("eager", dict(use_graph=False, wide_single_launch=False)), ("graph", dict(use_graph=True, wide_single_launch=False)),
                     ("single", dict(use_graph=False, wide_single_launch=True))):
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, discount=0.997, root_exploration_fraction=0.25,
                                 rng_mode=_rng(rng), **kw)
        m.seed(np.arange(B, dtype=np.uint64) + 9)
        e = m.run(obs, heads, train=train)
        assert (m._graph is not None) == (name == "graph")
        assert e.last_kernel().startswith("k_search_mlp_wide<") == (name == "single"), (name, e.last_kernel())
        action, policy, cv, rv2 = (t.clone() for t in e.act(1.0))
        visits, priors, rv, cr = e.root_stats()
        torch.cuda.synchronize()
        out = [t.cpu().numpy().copy() for t in (visits, priors, rv, cr, action, policy, cv, rv2)]
        res[name] = (out, _snapshot(e, rng, sorted({0, B // 2, B - 1})))
    return res


@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_wide_searches_with_the_hip_root_agree_in_every_mode(rng):
    """(4,2,61,126,0), 68 trees x 11 simulations with hip_root heads: eager step-wise == graph replay == wide_single_launch,
    bit for bit in root statistics, act outputs, dumped trees and stream positions; in evaluation mode the engine's root priors
    are the policy `initial` wrote, through the reference's (p + 1e-12) / sum in float32."""
    shape, B, sims = (4, 2, 61, 126, 0), 68, 11
    model = _net(shape, 170, 3)
    heads = model.heads("cuda:0", hip_root=True)
    assert type(heads).__name__ == "HipMlpTileHeads" and heads.hip_root
    assert model.heads("cuda:0", hip_root=True) is heads and model.heads("cuda:0") is not heads
    obs = (torch.rand(B, 4, generator=torch.Generator().manual_seed(3)) - 0.5).mul(0.1).cuda().contiguous()
    res = _wide_runs(heads, B, sims, rng, obs)
    assert (res["eager"][0][0].sum(1) == sims).all()
    for other in ("graph", "single"):
        for a, b in zip(res["eager"][0], res[other][0]):
            assert np.array_equal(a, b), other
        _same_dumps(res["eager"][1][0], res[other][1][0])
        _same_states(res["eager"][1][1], res[other][1][1], rng)
    ev = _wide_runs(heads, B, sims, rng, obs, train=False)
    p0 = heads.initial(obs)[1].cpu().numpy()
    root64, _, bound = _references(model, obs.cpu(), shape[2])
    _held(f"wide search {rng} root policy", p0, root64["root_policy"], bound["policy"])
    p = p0 + np.float32(1e-12)
    want = (p / (p[:, 0] + p[:, 1])[:, None]).astype(np.float64)
    for name in ev:
        assert np.array_equal(ev[name][0][1], want), name


def _root_outputs_match(tag, model, shape, obs, rec):
    root64, _, bound = _references(model, obs.cpu(), shape[2])
    _root_matches(tag, shape, rec.root[0], rec.root[1], root64, bound)


@pytest.mark.parametrize("A,players", [(256, 1), (64, 2)], ids=["A256", "A64_two_players"])
def test_large_searches_with_the_hip_root(A, players):
    """(4,A,16,64,1) with backend="large", hip_root=True, 16 trees x 10 simulations, K = 3 -- at A = 256, and with two players
    at A = 64 (to_play alternating over the trees): the captured graph equals the eager run; a second engine fed the recorded
    head outputs builds the same trees and leaves the same stream positions; the recorded root outputs meet the bounds of the
    restatement test."""
    shape, B, sims, K = (4, A, 16, 64, 1), 16, 10, 3
    model = _net(shape, 180 + players, 4)
    heads = model.heads("cuda:0", backend="large", hip_root=True)
    assert type(heads).__name__ == "HipMlpLargeHeads" and heads.hip_root
    obs = torch.randn(B, 4, generator=torch.Generator().manual_seed(6)).cuda().contiguous()
    seeds = np.arange(B, dtype=np.uint64) + 5
    kw = dict(number_of_player=2) if players == 2 else {}
    run_kw = dict(to_play=np.arange(B, dtype=np.int32) % 2) if players == 2 else {}
    out = []
    for use_graph in (True, False):
        mc = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, maxium_action_sample=K, use_graph=use_graph, **kw)
        mc.seed(seeds)
        eng = mc.run(obs, heads, train=True, **run_kw)
        assert eng.large_actions and eng.A == A and (mc._graph is not None) == use_graph
        v, p, rv, cr = (x.clone() for x in eng.root_stats())
        out.append((v, p, rv, eng.act(1.0)[0].clone()))
        assert int(v.sum()) == B * sims
    for x, y in zip(*out):
        assert torch.equal(x, y)
    rec = _Recording(heads)
    _, eng = _search(B, rec, obs, seeds, sims, K, **kw, **run_kw)
    assert len(rec.rounds) == sims and getattr(eng, "n_cycle", 1) == players
    assert torch.equal(eng.root_stats()[0], out[1][0]) and torch.equal(eng.root_stats()[2], out[1][2])
    _, again = _search(B, _Tape(rec), obs, seeds, sims, K, **kw, **run_kw)
    _trees_equal(eng, again, B)
    _streams_equal(eng, again, B)
    _root_outputs_match(f"large search A{A} players {players} root", model, shape, obs, rec)


def test_defaults_are_unchanged_and_updated_weights_give_new_hip_root_heads():
    """Without the flag heads("cuda:0") and heads("cuda:0", backend="large") return evaluators whose `initial` is
    FusedMlpHeads.initial; one in-place update of the representation and the policy head gives new hip_root heads whose root
    outputs follow the updated net's restatement and differ from the old ones."""
    fused = _pkg("heads").FusedMlpHeads
    shape = (4, 2, 61, 126, 0)
    model = _net(shape, 190, 4)
    for kw, name in ((dict(), "HipMlpTileHeads"), (dict(backend="large"), "HipMlpLargeHeads")):
        plain = model.heads("cuda:0", **kw)
        assert type(plain).__name__ == name and not plain.hip_root
        assert plain.initial.__func__ is fused.initial and "initial" not in vars(plain)
        assert model.heads("cuda:0", hip_root=False, **kw) is plain
        flagged = model.heads("cuda:0", hip_root=True, **kw)
        assert flagged is not plain and type(flagged).__name__ == name and "initial" in vars(flagged)
    o = _obs(shape, 91, 64)
    od = o.cuda().contiguous()
    for kw in (dict(), dict(backend="large")):
        torch_root = [t.clone().cpu() for t in model.heads("cuda:0", **kw).initial(od)]
        root64, _, bound = _references(model, o, shape[2])
        _root_matches(f"torch root {kw}", shape, *torch_root, root64, bound)
    old = model.heads("cuda:0", hip_root=True)
    before = [t.clone().cpu() for t in old.initial(od)]
    with torch.no_grad():
        [m for m in model.prediction_function.policy if isinstance(m, torch.nn.Linear)][-1].bias.add_(torch.linspace(-1, 1, shape[1]))
        next(model.representation_function.parameters()).add_(0.01)
    new = model.heads("cuda:0", hip_root=True)
    assert new is not old and type(new).__name__ == "HipMlpTileHeads" and new.hip_root
    root64, _, bound = _references(model, o, shape[2])
    hid, pol = (t.clone().cpu() for t in new.initial(od))
    _root_matches("hip root after an in-place update", shape, hid, pol, root64, bound)
    assert not torch.equal(pol, before[1]) and not torch.equal(hid, before[0])


def test_refusals_on_the_device_side_of_the_suite():
    """hip_root=True with obs = 1025 raises ValueError naming the limit through Muzero.heads -- "auto" does not fall back to
    the torch heads, "large" does not either -- while the same nets without the flag build as before."""
    wide, large = mr.fresh_net(1025, 2, 61, 126, 0, seed=1), mr.fresh_net(1025, 200, 16, 64, 1, seed=1)
    assert type(wide.heads("cuda:0")).__name__ == "HipMlpTileHeads"
    assert type(large.heads("cuda:0", backend="large")).__name__ == "HipMlpLargeHeads"
    with pytest.raises(ValueError, match="1024"):
        wide.heads("cuda:0", hip_root=True)
    with pytest.raises(ValueError, match="1024"):
        large.heads("cuda:0", backend="large", hip_root=True)
    # an evaluator the flag does not concern ignores it
    small = mr.fresh_net(4, 2, 31, 64, 0, seed=1)
    assert type(small.heads("cuda:0", hip_root=True)).__name__ == "HipMlpHeads"
