"""The HIP vision_model head kernels (csrc/smz_vision.hip, csrc/smz_vision_device.hpp) and their matrix-core twin in the
single-launch search (csrc/smz_vision_search.hip) over the whole envelope smz_vision_layout accepts, against the float64
restatement of tests/vision_reference.py (anchored to the reference's own numbers by tests/test_vision_reference.py).

Shapes (A, S, H, L), each with the path it is the first to run (n = up4(H) / 4 groups of four inputs of an H-wide layer, summed
by dense_stream as four quarters of pl = ceil(n / 4) groups):
  (1,1,1,0)     every dimension 1: n = 1, three empty quarters; S = 1 decode; A = 1 policy is exactly 1
  (2,31,64,1)   the fixtures' shape under the rule below (anchor)
  (3,5,7,2)     H not a multiple of 4; n = 2: quarters 1,1,0,0
  (5,12,17,1)   n = 5, pl = 2: quarters 2,2,1,0
  (4,32,20,0)   L = 0: no mid layer, no residual block; S at the search limit, even
  (2,8,36,3)    n = 9, pl = 3: quarters 3,3,3,0; L = 3
  (7,21,52,1)   n = 13, pl = 4: quarters 4,4,4,1
  (33,64,63,2)  A > 32, S = 64, one padded input
  (64,64,64,0)  every limit: all 64 lanes in softmax and decode
  (2,2,64,6)    L = 6 (the layout bounds L only below)
Gains (vision_reference.fresh_net: the last Linear of every tower): 1 = a fresh net, 4, 16 = |logit| up to 16.

The comparison rule.  The per-pixel min-max scaling divides by the channel span of ONE pixel; on these nets up to 72 % of the
pixels of a case have a span of exactly 0 and hundreds a span below 1e-3, where the float32 torch modules themselves are up to
1.3e-3 from their float64 copies on the scaled plane.  So
  hidden planes (root and recurrent) are judged on max |got - want64| * max(span64, 1e-5), span64 = the float64 span of the
    pixel before scaling: it undoes the division.  Pixels with 0.5e-5 <= span64 <= 2e-5 sit on the + 1e-5 discontinuity and
    are left out (asserted: at most 1 % of a case; pixels of span exactly 0 stay in).  Bound: 4 x max(e32w of the case, largest
    e32w of any shape at that gain), e32w = the same statistic of the float32 restatement, computed here on the CPU: a
    property of the reference arithmetic, never of the kernels.  The factor 4 is that of the sibling envelope files; it covers
    the kernels' own associations (three tap-row chains combined as (r0 + r1) + r2, fused multiply-adds, four-quarter tower
    sums).  A wrong tap, channel, batch-norm term or action plane shows at 1e-3 and above.
  policies and values are judged on the prediction stage alone: the reference is Restatement.predict of THE KERNEL'S OWN
    hidden output cast to float64 (the kernel hands the registers it stores to its prediction stage).  Policy bound
    max(1e-6, 4 x e32), e32 = the float32 against the float64 prediction of the same rows; decoded values within
    golden_util.DECODE_BOUND_STEPS stairs, with the gain-16 widening of test_gpu_lstm_envelope._decoded.
  rewards read the parent only: Restatement.transition of the inputs under the same rule; afterstate rows are exactly 0.

With SMZ_TOLERANCE_LOG set, every comparison appends its largest error (profiles/vision_envelope_tolerances.jsonl is one run).
Measured on MI355X: see test_hip_vision_heads_match_the_float64_restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu  # noqa: F401
import vision_reference as vr
from search_helpers import _pkg, _same_dumps, _same_states, _snapshot
from test_gpu_lstm import _FakeEngine, _held
from test_gpu_lstm_envelope import GUARD_ROWS, NAN_BITS, _decoded, _guarded, _untouched  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES, GAINS = vr.SHAPES, vr.GAINS
FACTOR = 4
POLICY_ATOL = 1e-6
SEARCH_SHAPES = ((3, 5, 7, 2), (4, 32, 20, 0), (2, 8, 36, 3), (2, 21, 52, 1))


def _layout(shape):
    lib_mod = _pkg("_lib")
    d = lib_mod.VisionDesc(*shape)
    return lib_mod.load().smz_vision_layout(C.byref(d)), d


def _engine_rows(h, a, br):
    fe = _FakeEngine()
    fe.parent_hidden = torch.as_tensor(h, dtype=torch.float32).cuda().contiguous()
    fe.last_action = torch.as_tensor(a).int().cuda()
    fe.branch = torch.as_tensor(br).to(torch.uint8).cuda()
    fe.B, fe.S = fe.parent_hidden.shape[0], 147
    return fe


def _hidden(what, got, ref64, e32w, floor):
    """Span-weighted comparison of a hidden plane (module docstring); the share of left-out pixels is logged and held to 1 %."""
    err, seam = vr.span_weighted(got, ref64["hidden"], ref64["span"])
    bound = FACTOR * max(e32w, floor)
    print(f"{what}: span-weighted {float(err.max()):.3e} of {bound:.3e} ({float(err.max()) / bound:.3f}); left out {100 * seam:.4f} %")
    _held(what + " left-out share", [seam], [0.0], 0.01)
    _held(what + " span-weighted", err.numpy(), np.zeros(1), bound)


def _prediction(what, r64, r32, hidden, branch, got_policy, got_value, gain):
    """Policy and decoded value against the prediction stage alone, evaluated on the hidden rows the heads produced."""
    h = hidden.double()
    p64, p32 = r64.predict(h, branch), r32.predict(h, branch)
    e32 = float((p32["policy"].double() - p64["policy"]).abs().max())
    bound = max(POLICY_ATOL, FACTOR * e32)
    err = float((got_policy.double() - p64["policy"]).abs().max())
    print(f"{what} policy: {err:.3e} of {bound:.3e} ({err / bound:.3f})")
    _held(what + " policy", got_policy, p64["policy"], bound)
    if got_value is not None:
        _decoded(what + " value", got_value, p64, p32, "value", gain, torch.ones(len(h), dtype=torch.bool))


def _compare(tag, c, heads, gain, rows=None):
    """One case of vision_reference.case through `heads` (the first `rows` frames and recurrent rows of it)."""
    f, h, a, br = c["inputs"]
    nf, n = (len(f), len(h)) if rows is None else (min(rows, len(f)), rows)
    cut = lambda d, k: {key: v[:k] for key, v in d.items()}
    root64, out64, out32 = cut(c["root64"], nf), cut(c["out64"], n), cut(c["out32"], n)
    floor = vr.floor_of(gain)
    hid, pol = (t.clone().cpu() for t in heads.initial(f[:nf].cuda().contiguous()))
    h2, rw, p2, v2 = (t.clone().cpu() for t in heads.recurrent(_engine_rows(h[:n], a[:n], br[:n])))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (hid, pol, h2, rw, p2, v2))
    assert hid.shape == (nf, 147) and h2.shape == (n, 147) and pol.shape == (nf, c["r64"].A) and p2.shape == (n, c["r64"].A)
    _hidden(f"{tag} root hidden", hid, root64, c["e32w"]["root_hidden"], floor["root_hidden"])
    _hidden(f"{tag} hidden", h2, out64, c["e32w"]["hidden"], floor["hidden"])
    _prediction(f"{tag} root", c["r64"], c["r32"], hid, torch.ones(nf), pol, None, gain)
    _prediction(f"{tag} recurrent", c["r64"], c["r32"], h2, br[:n], p2, v2, gain)
    if c["r64"].A == 1:
        assert (pol == 1).all() and (p2 == 1).all()
    dyn = br[:n] != 0
    assert (rw[~dyn] == 0).all()
    if bool(dyn.any()):
        _decoded(f"{tag} reward", rw, out64, out32, "reward", gain, dyn)


def test_every_shape_is_accepted_by_the_layout():
    assert len(SHAPES) == 10
    for shape in SHAPES:
        rc, d = _layout(shape)
        assert rc == 0, shape
        assert all(o % 4 == 0 for o in d.off) and d.total_floats % 4 == 0, shape
        assert 0 < d.small_floats <= 1280 and d.OP == 64, (shape, d.small_floats, d.OP)
        assert (d.A, d.S, d.H, d.L) == shape


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=vr.shape_id)
def test_hip_vision_heads_match_the_float64_restatement(shape, gain):
    """32 frames and 2048 recurrent rows of mixed branches per shape and gain, judged by the rule of the module docstring.
    Measured on MI355X at the first run, worst over the ten shapes (gain 1 / 4 / 16; the hidden planes do not depend on the gain):
    root hidden planes, span-weighted, 4.9e-7 at (2,2,64,6) = 0.20 of its bound 2.5e-6; recurrent hidden planes 1.19e-6 at
    (2,8,36,3) = 0.245 of 4.9e-6 -- the kernels are as near to float64 as the float32 torch modules are (e32w there 1.22e-6), so
    the factor stays at 4; root policies 5.5e-8 / 1.3e-7 / 1.8e-7 and recurrent policies 6.3e-8 / 1.3e-7 / 3.2e-7 (0.26 of the
    bound 1.24e-6 at (4,32,20,0), the only case whose 4 x e32 exceeds 1e-6); decoded values 0.75 / 0.74 / 0.83 stairs and
    rewards 0.75 / 0.75 / 0.78 stairs of 1.05 (no row needed the gain-16 widening); pixels left out at most 0.005 % of a
    case ((33,64,63,2)).  Worst ratio of kernel error to bound per output: root hidden 0.20, hidden 0.245, root policy 0.18,
    policy 0.26, value 0.79, reward 0.74."""
    c = vr.case(shape, gain)
    heads = c["model"].heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipVisionHeads" and (heads.A, heads.Ssup, heads.H, heads.L) == shape
    _compare(f"envelope {vr.shape_id(shape)} gain {gain}", c, heads, gain)


@pytest.mark.parametrize("mode", ["dynamics", "afterstate"])
def test_rows_of_one_branch_only(mode):
    """(5,12,17,1) at gain 4 with every row on the dynamics pair, and with every row on the afterstate pair: no workgroup has
    a wavefront of the other branch beside it."""
    shape, gain = (5, 12, 17, 1), 4
    c = vr.case(shape, gain, mode=mode)
    heads = c["model"].heads("cuda:0", backend="hip")
    assert bool((c["inputs"][3] == (1 if mode == "dynamics" else 0)).all())
    _compare(f"envelope {vr.shape_id(shape)} gain {gain} all {mode}", c, heads, gain)


def test_small_spans_of_both_kinds_occur_in_the_cases():
    """The span-weighted rule is exercised: the cases hold pixels of span exactly 0 and pixels with spans of 1e-5 .. 1e-3."""
    spans = torch.cat([vr.case(s, 1)[k]["span"].flatten() for s in SHAPES for k in ("root64", "out64")])
    assert int((spans == 0).sum()) > 100 and int(((spans > 1e-5) & (spans < 1e-3)).sum()) > 10


@pytest.mark.parametrize("shape", [(5, 12, 17, 1), (64, 64, 64, 0)], ids=vr.shape_id)
def test_rows_do_not_depend_on_the_launch_geometry_and_nothing_else_is_written(shape):
    """smz_vision_recurrent / smz_vision_initial through ctypes on the test's own buffers.  Recurrent: B on both sides of a
    ragged last workgroup (four wavefronts of one row each) and parent rows 147 and 160 floats apart, the 13 padding floats
    holding NaN: rows < B are bit for bit those of the B = 4097, ld = 147 launch, and the 8 guard rows behind row B - 1 of
    all four outputs keep their NaN pattern.  Initial: B = 1 and 3 likewise.  ld = 146 and B = 0 are refused before a launch."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    A, S, H, L = shape
    c = vr.case(shape, 4)
    heads = c["model"].heads("cuda:0", backend="hip")
    big = 4097
    g = torch.Generator().manual_seed(77)
    h_all = torch.rand(big, 147, generator=g)
    a_all = torch.randint(0, A, (big,), generator=g).int().cuda()
    br_all = torch.randint(0, 2, (big,), generator=g).to(torch.uint8).cuda()
    f_all = torch.rand(3, 3, 98, 98, generator=g).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    widths = dict(hidden=147, reward=1, policy=A, value=1)

    def recurrent(n, ld, rc_want=0):
        x = torch.full((max(n, 1), max(ld, 147)), float("nan"))       # (a refused ld is never read)
        x[:, :147] = h_all[:max(n, 1)]
        x, a, br = x.cuda(), a_all[:max(n, 1)].clone(), br_all[:max(n, 1)].clone()
        out = {k: _guarded(n, w) for k, w in widths.items()}
        rc = lib.smz_vision_recurrent(C.byref(heads.desc), p(heads.weights), p(x), ld, p(a), p(br), p(out["hidden"]),
                                      p(out["reward"]), p(out["policy"]), p(out["value"]), n, stream)
        torch.cuda.synchronize()
        assert rc == rc_want, (n, ld, rc)
        for k, w in widths.items():
            assert _untouched(out[k], n if rc == 0 else 0, w), (n, ld, k)
        return {k: out[k][:n * w].cpu() for k, w in widths.items()}

    def initial(n, rc_want=0):
        out = dict(hidden=_guarded(n, 147), policy=_guarded(n, A))
        rc = lib.smz_vision_initial(C.byref(heads.desc), p(heads.weights), p(f_all), p(out["hidden"]), p(out["policy"]), n, stream)
        torch.cuda.synchronize()
        assert rc == rc_want, (n, rc)
        for k, w in (("hidden", 147), ("policy", A)):
            assert _untouched(out[k], n if rc == 0 else 0, w), (n, k)
        return {k: out[k][:n * w].cpu() for k, w in (("hidden", 147), ("policy", A))}

    want = recurrent(big, 147)
    assert not any(bool((v == NAN_BITS).any()) for v in want.values())
    assert all(bool(torch.isfinite(v.view(torch.float32)).all()) for v in want.values())
    for ld in (147, 160):
        for n in (1, 3, 4, 5, big):
            if (n, ld) == (big, 147):
                continue
            got = recurrent(n, ld)
            for k, v in got.items():
                assert torch.equal(v, want[k][:v.numel()]), (n, ld, k)
    root = initial(3)
    assert all(bool(torch.isfinite(v.view(torch.float32)).all()) for v in root.values())
    for k, v in initial(1).items():
        assert torch.equal(v, root[k][:v.numel()]), k
    recurrent(5, 146, rc_want=lib_mod.SMZ_ERR_INVALID)
    recurrent(0, 147, rc_want=lib_mod.SMZ_ERR_INVALID)
    initial(0, rc_want=lib_mod.SMZ_ERR_INVALID)


@pytest.mark.parametrize("shape", SEARCH_SHAPES, ids=vr.shape_id)
def test_single_launch_vision_search_equals_stepwise_at_small_widths(shape):
    """k_search_vision (towers of the workgroup's four leaves on the matrix cores, quarters of plh4 inputs) against the step-wise
    kernels (dense_stream: four k-ordered fma chains over the same quarters) where the quarters are ragged or empty -- H = 7,
    20, 36, 52 -- on perturbed nets at gain 4: 37 trees, 12 simulations; root statistics, act, three dumped trees and the
    stream positions are equal bit for bit."""
    mcts_mod = _pkg("mcts")
    A, S, H, L = shape
    model = vr.fresh_net(A, S, H, L, seed=600 + SEARCH_SHAPES.index(shape), gain=4)
    heads = model.heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipVisionHeads" and (heads.A, heads.Ssup, heads.H, heads.L) == shape
    B, sims = 37, 12
    obs = torch.rand(B, 3, 98, 98, generator=torch.Generator().manual_seed(5)).cuda()
    trees, res = (0, B // 2, B - 1), []
    for single in (True, False):
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, discount=0.997, root_exploration_fraction=0.25,
                                 use_graph=False, single_launch=single)
        m.seed(np.arange(B, dtype=np.uint64) + 21)
        e = m.run(obs, heads, train=True)
        assert m._single is (True if single else None)
        if single:
            assert e.last_kernel().startswith("k_search_vision<"), e.last_kernel()
        visits, priors, rv, cr = e.root_stats()
        action, policy, cv, _ = e.act(0.5)
        torch.cuda.synchronize()
        res.append(([t.cpu().numpy().copy() for t in (visits, priors, rv, cr, action, policy, cv)], _snapshot(e, "mt19937", trees)))
    assert (res[0][0][0].sum(1) == sims).all() and np.isfinite(res[0][0][2]).all()
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    _same_dumps(res[0][1][0], res[1][1][0])
    _same_states(res[0][1][1], res[1][1][1], "mt19937")


def test_shapes_outside_the_envelope_are_refused():
    """smz_vision_layout says SMZ_ERR_INVALID for A, S or H at 0 and at 65 and for L = -1; heads(backend="hip") raises for
    H = 65; heads(backend="auto") hands out the torch modules (ModuleHeads) for H = 65 and for A = 65, which meet the bounds
    of the module docstring on 256 rows at gain 1 (measured: hidden planes, span-weighted, 2.5e-7 root and recurrent, policies
    6.2e-8, decoded scalars 0.74 stairs) and search step-wise; the single-launch entry point refuses a descriptor of such a
    shape as it refuses any descriptor that smz_vision_layout does not reproduce."""
    lib_mod, mcts_mod, eng_mod = _pkg("_lib"), _pkg("mcts"), _pkg("engine")
    lib = lib_mod.load()
    for bad in ((0, 31, 64, 1), (65, 31, 64, 1), (2, 0, 64, 1), (2, 65, 64, 1), (2, 31, 0, 1), (2, 31, 65, 1), (2, 31, 64, -1)):
        assert _layout(bad)[0] == lib_mod.SMZ_ERR_INVALID, bad
    for n, shape in enumerate(((2, 31, 65, 1), (65, 31, 64, 1))):
        model = vr.fresh_net(*shape, seed=700 + n, gain=1)
        if n == 0:
            with pytest.raises(ValueError):
                model.heads("cuda:0", backend="hip")
        heads = model.heads("cuda:0", backend="auto")
        assert type(heads).__name__ == "ModuleHeads" and heads.is_rgb and getattr(heads, "single_launch", None) is None
        rows = 256
        g = torch.Generator().manual_seed(90 + n)
        f, h = torch.rand(8, 3, 98, 98, generator=g), torch.rand(rows, 147, generator=g)
        a, br = torch.randint(0, shape[0], (rows,), generator=g), torch.randint(0, 2, (rows,), generator=g)
        r64, r32 = vr.Restatement(model), vr.Restatement(model, torch.float32)
        c = dict(model=model, inputs=(f, h, a, br), r64=r64, r32=r32, root64=r64.represent(f), out64=r64.transition(h, a, br),
                 out32=r32.transition(h, a, br))
        c["e32w"] = dict(root_hidden=float(vr.span_weighted(r32.represent(f)["hidden"], c["root64"]["hidden"], c["root64"]["span"])[0].max()),
                         hidden=float(vr.span_weighted(c["out32"]["hidden"], c["out64"]["hidden"], c["out64"]["span"])[0].max()))
        _compare(f"refused {vr.shape_id(shape)} torch modules", c, heads, 1)
        # a search with them runs on the step-wise kernels
        B, sims = 8, 4
        m = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, discount=0.997, root_exploration_fraction=0.25,
                                 use_graph=False)
        m.seed(np.arange(B, dtype=np.uint64))
        e = m.run(f.cuda(), heads, train=True)
        visits = e.root_stats()[0]
        torch.cuda.synchronize()
        assert m._single is None and (visits.cpu().numpy().sum(1) == sims).all()
    # ... and the single-launch entry point refuses a descriptor of such a shape before any launch
    good = vr.net_of((2, 31, 64, 1), 1).heads("cuda:0", backend="hip")
    eng = eng_mod.SearchEngine(8, 2, 147, num_simulations=4)
    h0, p0 = (t.clone() for t in good.initial(torch.rand(8, 3, 98, 98, generator=torch.Generator().manual_seed(1)).cuda()))
    for shape in ((2, 31, 65, 1), (65, 31, 64, 1)):
        d = type(good.desc).from_buffer_copy(good.desc)
        d.A, d.S, d.H, d.L = shape
        rc = lib.smz_search_vision(eng.h, C.byref(d), C.c_void_p(good.weights.data_ptr()), C.c_void_p(h0.data_ptr()),
                                   C.c_void_p(p0.data_ptr()), 0, None)
        assert rc == lib_mod.SMZ_ERR_INVALID and eng.last_kernel() == "", (shape, rc)
        assert lib.smz_last_error().decode() == "smz_search_vision: descriptor does not describe a vision_model weight buffer"
    eng.close()
