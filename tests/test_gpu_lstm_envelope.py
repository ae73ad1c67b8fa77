"""The HIP lstm_model head kernels (csrc/smz_lstm.hip) over the whole envelope smz_lstm_layout accepts, against the float64
restatement of tests/lstm_reference.py (anchored to the reference's own numbers by tests/test_lstm_reference.py).

What each shape is there for (first shape that runs the path):
  gate_columns<3> (3 O > 128)                  (7,64,8,2): policy trunks, A = 64;  (4,2,43,1): state trunks, S = 43
  gate_columns<1> on state trunks (S <= 21)   (1,1,1,1), (1,1,1,4), (5,3,4,4), (3,2,5,3), (8,4,21,2), (7,64,8,2), (4,16,16,4),
                                               (4,7,20,3), (300,5,21,1), (4096,2,16,1);  <2> on both trunk kinds: (6,22,22,1)
  dense(): no tail (K4 / 4 a multiple of 4)    (4,18,32,1): S = 32 -> 8 groups;  (4,16,16,4): 4 groups;  (4096,2,16,1): 1024
  dense(): no unrolled body (K4 / 4 < 4)       (1,1,1,1): 1 group;  (5,3,4,4): 2 and 1;  (3,2,5,3): 2
  dense(): body + tail                         (4,2,31,1): 9 = 8 + 1 .. (9,4,48,1): 13 = 12 + 1;  (300,5,21,1): 75 = 72 + 3
  reads past a matrix, smallest G              (1,1,1,1) / (1,1,1,4): A = 1 -> G = 3, 244 floats past the matrix, and the last
                                               layer of trunk 6 / the representation matrix at the end of the image (every shape)
  L = 3, 4                                     (3,2,5,3), (4,7,20,3);  (1,1,1,4), (5,3,4,4), (4,16,16,4)
  S = 1 (span 0 -> + 1e-5), S even, A >= S     (1,1,1,1);  (5,3,4,4), (4,18,32,1), ...;  (6,22,22,1), (4,33,33,1), (7,64,8,2)
  k_lstm_initial above 64 KB of dynamic LDS    (4096,2,16,1): 70,656 B of scratch;  obs not a multiple of 4: (1,..), (5,..), (3,..),
                                               (6,..), (7,..), (9,..), and (300,5,21,1) with a long body
  one workgroup per CU                         (9,4,48,1): 159,712 B
Gains (lstm_reference.fresh_net): 1 = a fresh net (Taylor branch of lstm_tanh), 4 = pre-activations around the 0.5 seam,
16 = saturated gates (|logit| up to tanh(1) * sigmoid(large) = 0.76).

Tolerances: DESIGN.md 1 as in test_gpu_lstm.py -- 1e-5 on hidden rows, 1e-6 on policies, decoded scalars within
golden_util.DECODE_BOUND_STEPS stairs of the float64 decode of the float64 logits -- unchanged at gains 1 and 4.  At gain 16
float32 itself leaves that contract (torch CPU float32 modules against float64 on these nets and rows: up to 2.7e-5 on hidden
rows and 5.6e-6 on policies, both at (4,16,16,4)), so there the bound of an output is max(contract, 4 x e32), e32 = the largest error of
the float32 MODULES against the float64 restatement on the same rows, computed here on the CPU: a property of the reference
arithmetic, never of the kernels.  The factor 4 covers the kernels' legitimately different roundings (folded input layer,
packed even / odd accumulation, hardware exp), each of the order of e32; a wrong column or a dropped input group shows at
1e-3 and above.  Decoded scalars at gain 16: when the float32 modules' own logits already move a row by more than
DECODE_BOUND_STEPS stairs, every row's bound is widened by the stairs that 4 x e32 on its logits amounts to, to first order:
|dy| <= 4 e32 sum_k p_k |k - y| for the support expectation y, and one stair is DECODE_STEP sqrt(1 + 0.004 (|y| + 1.001)) / 2
wide in y.

With SMZ_TOLERANCE_LOG set, every comparison appends its largest error (profiles/lstm_envelope_tolerances.jsonl is one run)."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as gu
import lstm_reference as lr
from test_gpu_lstm import _FakeEngine, _engine_rows, _held  # noqa: F401

pytestmark = pytest.mark.gpu

LDS_BUDGET = 160 * 1024
# (obs, A, S, L): LDS bytes of one smz_lstm_recurrent workgroup
SHAPES = {(1, 1, 1, 1): 6656, (1, 1, 1, 4): 8000, (5, 3, 4, 4): 13184, (3, 2, 5, 3): 15392, (4, 2, 31, 1): 74224,
          (8, 4, 21, 2): 75536, (6, 22, 22, 1): 68944, (4, 18, 32, 1): 107648, (4, 33, 33, 1): 147840, (7, 64, 8, 2): 148032,
          (4, 16, 16, 4): 107264, (4, 7, 20, 3): 94576, (4, 2, 43, 1): 131440, (9, 4, 48, 1): 159712, (300, 5, 21, 1): 44144,
          (4096, 2, 16, 1): 25920}
# refused: trunks + scratch beyond the budget (bytes), or a dimension outside the layout's limits (None)
REFUSED = {(9, 4, 49, 1): 175024, (4, 2, 31, 3): 197616, (4, 2, 64, 1): 269184, (4, 65, 8, 1): None, (4, 2, 8, 5): None,
           (4097, 2, 8, 1): None}
GAINS = (1, 4, 16)
B = 4096
HIDDEN_ATOL, POLICY_ATOL = 1e-5, 1e-6


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _layout(shape):
    lib_mod = _pkg("_lib")
    d = lib_mod.LstmDesc(*shape)
    return lib_mod.load().smz_lstm_layout(C.byref(d)), d


def _id(shape):
    return "x".join(str(v) for v in shape)


def _inputs(shape, seed):
    obs, A, S, _ = shape
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(B, obs, generator=g) - 0.5
    h = torch.rand(B, S, generator=g)
    a = torch.randint(0, A, (B,), generator=g)
    br = torch.randint(0, 2, (B,), generator=g)
    assert 0.4 < float(br.float().mean()) < 0.6
    return o, h, a, br


def _e32(ref64, ref32, keys):
    return {k: float((ref64[k] - ref32[k].double()).abs().max()) for k in keys}


def _hidden_rows(span, S):
    """Rows of the hidden comparison: those at the + 1e-5 discontinuity of the scaling may be left out, at most 1 %."""
    keep = ~((span >= 0.5e-5) & (span <= 2e-5))
    assert float((~keep).float().mean()) <= 0.01
    if S == 1:
        assert (span == 0).all()
    return keep


def _stairs_of(logits64, delta):
    """Stairs that an error of `delta` on every logit of a row amounts to (first order; module docstring)."""
    S = logits64.shape[1]
    p = torch.softmax(logits64, 1)
    k = torch.arange(-(S // 2), -(S // 2) + S, dtype=torch.float64)
    y = (k * p).sum(1)
    dy = delta * (p * (k - y[:, None]).abs()).sum(1)
    return (2 * dy / (torch.sqrt(1 + 4 * 0.001 * (y.abs() + 1 + 0.001)) * gu.DECODE_STEP)).numpy()


def _decoded(what, got, ref64, ref32, key, gain, rows):
    """Decoded reward / value against the float64 decode of the float64 logits, in stairs (`rows`: the rows that have logits --
    an afterstate row's reward is 0 on both sides)."""
    want = ref64[key].numpy()
    steps = gu.decode_steps(got.cpu().numpy(), want)
    widen = np.zeros_like(steps)
    if gain == 16:
        logits64, logits32 = ref64[key + "_logits"], ref32[key + "_logits"].double()
        floor = gu.decode_steps(lr.decode(logits32).numpy(), want)[rows.numpy()]
        if floor.max() > gu.DECODE_BOUND_STEPS:
            widen = _stairs_of(logits64, 4 * float((logits64 - logits32).abs().max()))
    # the row nearest to its own bound stands for all rows: logged are its stairs and its bound
    i = int(np.argmax(steps / (gu.DECODE_BOUND_STEPS + widen)))
    print(f"{what}: {steps.max():.3f} stairs at most; row {i}: {steps[i]:.3f} of {gu.DECODE_BOUND_STEPS + widen[i]:.3f}")
    _held(what + " stairs", steps[i:i + 1], np.zeros(1), float(gu.DECODE_BOUND_STEPS + widen[i]))


def _compare(tag, shape, gain, heads, model, seed, hidden_atol=HIDDEN_ATOL, policy_atol=POLICY_ATOL):
    obs, A, S, _ = shape
    o, h, a, br = _inputs(shape, seed)
    r64 = lr.Restatement(model)
    root64, out64 = r64.initial(o), r64.recurrent(h, a, br)
    root32 = out32 = None
    bound = dict(root_hidden=hidden_atol, hidden=hidden_atol, root_policy=policy_atol, policy=policy_atol)
    if gain == 16:
        r32 = lr.Restatement(model, torch.float32)
        root32, out32 = r32.initial(o), r32.recurrent(h, a, br)
        e32 = dict(_e32(root64, root32, ("root_hidden", "root_policy")), **_e32(out64, out32, ("hidden", "policy")))
        bound = {k: max(v, 4 * e32[k]) for k, v in bound.items()}
    hid, pol = (t.clone() for t in heads.initial(o.cuda().contiguous()))
    fe = _engine_rows(h, a, br, A)
    h2, rw, p2, v2 = (t.clone() for t in heads.recurrent(fe))
    torch.cuda.synchronize()
    for key, got, ref, span in (("root_hidden", hid, root64, root64["root_span"]), ("hidden", h2, out64, out64["span"])):
        keep = _hidden_rows(span, S)
        if S == 1:      # span exactly 0 on both sides: (x - x) / 1e-5
            assert (got.cpu() == 0).all() and (ref[key] == 0).all()
        _held(f"{tag} {key}", got.cpu()[keep], ref[key][keep], bound[key])
    _held(f"{tag} root_policy", pol.cpu(), root64["root_policy"], bound["root_policy"])
    _held(f"{tag} policy", p2.cpu(), out64["policy"], bound["policy"])
    assert (rw.cpu()[br == 0] == 0).all()
    _decoded(f"{tag} reward", rw, out64, out32, "reward", gain, br != 0)
    _decoded(f"{tag} value", v2, out64, out32, "value", gain, torch.ones_like(br, dtype=torch.bool))


def test_every_shape_of_the_envelope_is_accepted_by_the_layout():
    assert len(SHAPES) == 16
    for shape, lds in SHAPES.items():
        rc, d = _layout(shape)
        assert rc == 0 and d.lds_bytes == lds <= LDS_BUDGET, (shape, rc, d.lds_bytes)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", list(SHAPES), ids=_id)
def test_hip_lstm_heads_match_the_float64_restatement(shape, gain):
    """4096 observations and 4096 recurrent rows of mixed branches per shape and gain.  Measured on MI355X, worst over the
    sixteen shapes (gain 1 / 4 / 16): root hidden rows 1.7e-6 / 1.7e-6 / 1.7e-6 (obs 4096), root policies 7.2e-8 / 3.1e-7 /
    3.3e-6 (bound there 6.4e-6), hidden rows 4.8e-7 / 4.1e-7 / 1.3e-5 (at (7,64,8,2), bound there 7.8e-5), policies 7.4e-8 /
    1.1e-7 / 4.4e-6 (at (4,16,16,4), bound there 2.2e-5); decoded scalars 0.75 / 0.75 / 0.76 stairs from the float64 decode.
    The widening of the module docstring applied once: the values of (4,16,16,4) at gain 16, where the float32 modules' own
    logits leave the bound, were up to 3.68 stairs away against a per-row widening of up to 145 stairs; no row of any case
    sat at the + 1e-5 discontinuity of the scaling (S = 1: span 0 and scaled state 0 on both sides)."""
    obs, A, S, L = shape
    model = lr.fresh_net(obs, A, S, L, seed=100 + list(SHAPES).index(shape), gain=gain)
    heads = model.heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipLstmHeads"
    _compare(f"envelope {_id(shape)} gain {gain}", shape, gain, heads, model, seed=7 + list(SHAPES).index(shape))


NAN_BITS = 0x7FC00ABC
GUARD_ROWS = 8


def _guarded(rows, width):
    return torch.full(((rows + GUARD_ROWS) * width,), NAN_BITS, dtype=torch.int32, device="cuda")


def _untouched(buf, rows, width):
    return bool((buf[rows * width:] == NAN_BITS).all())


@pytest.mark.parametrize("shape", [(4, 2, 31, 1), (9, 4, 48, 1)], ids=_id)
def test_rows_do_not_depend_on_the_launch_geometry_and_nothing_else_is_written(shape):
    """smz_lstm_initial / smz_lstm_recurrent through ctypes on the test's own buffers, B on both sides of every change of
    rows_per_wave (2048 waves: 1 row up to 2048, 2 up to 4096, then 3): the 8 guard rows behind row B - 1 of every output
    keep their NaN pattern, rows < B are bit for bit those of the B = 4097 launch (whichever wave and slot computed them),
    and a call without a reward buffer leaves the other three outputs bit for bit the same."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    obs, A, S, L = shape
    model = lr.fresh_net(obs, A, S, L, seed=31, gain=4)
    heads = model.heads("cuda:0", backend="hip")
    big = 4097
    g = torch.Generator().manual_seed(77)
    o_all = (torch.rand(big, obs, generator=g) - 0.5).cuda()
    x_all = torch.cat([torch.rand(big, S, generator=g),
                       torch.nn.functional.one_hot(torch.randint(0, A, (big,), generator=g), A).float()], 1).cuda()
    br_all = torch.randint(0, 2, (big,), generator=g).to(torch.uint8).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def launch(n, with_reward=True):
        o, x, br = o_all[:n].clone(), x_all[:n].clone(), br_all[:n].clone()
        widths = dict(root_hidden=S, root_policy=A, hidden=S, reward=1, policy=A, value=1)
        out = {k: _guarded(n, w) for k, w in widths.items()}
        lib_mod.check(lib.smz_lstm_initial(C.byref(heads.desc), p(heads.weights), p(o), p(out["root_hidden"]),
                                           p(out["root_policy"]), n, stream))
        lib_mod.check(lib.smz_lstm_recurrent(C.byref(heads.desc), p(heads.weights), p(x), p(br), p(out["hidden"]),
                                             p(out["reward"]) if with_reward else None, p(out["policy"]), p(out["value"]), n,
                                             stream))
        torch.cuda.synchronize()
        for k, w in widths.items():
            assert _untouched(out[k], n if (with_reward or k != "reward") else 0, w), (n, k)
        return {k: out[k][:n * w].cpu() for k, w in widths.items()}

    want = launch(big)
    assert not any(bool((v == NAN_BITS).any()) for v in want.values())
    assert torch.isfinite(want["hidden"].view(torch.float32)).all() and torch.isfinite(want["value"].view(torch.float32)).all()
    for n in (1, 3, 5, 2047, 2048, 2049):
        got = launch(n)
        for k, v in got.items():
            assert torch.equal(v, want[k][:v.numel()]), (n, k)
    got = launch(2049, with_reward=False)
    for k in ("root_hidden", "root_policy", "hidden", "policy", "value"):
        assert torch.equal(got[k], want[k][:got[k].numel()]), k


@pytest.mark.parametrize("shape", list(REFUSED), ids=_id)
def test_shapes_outside_the_envelope_are_refused_and_fall_back_to_the_torch_heads(shape):
    """smz_lstm_layout says SMZ_ERR_INVALID, heads(backend="hip") raises, heads(backend="auto") hands out LstmTorchHeads; for
    the two shapes nearest to the budget those torch heads meet the gain-1 tolerances against the restatement (measured:
    hidden rows 2.7e-7, policies 6.3e-8, decoded scalars 0.74 stairs)."""
    lib_mod = _pkg("_lib")
    rc, d = _layout(shape)
    assert rc == lib_mod.SMZ_ERR_INVALID
    if REFUSED[shape] is not None:
        assert d.lds_bytes == REFUSED[shape] > LDS_BUDGET
    obs, A, S, L = shape
    model = lr.fresh_net(obs, A, S, L, seed=200 + list(REFUSED).index(shape), gain=1)
    with pytest.raises(ValueError):
        model.heads("cuda:0", backend="hip")
    heads = model.heads("cuda:0", backend="auto")
    assert type(heads).__name__ == "LstmTorchHeads"
    if list(REFUSED).index(shape) < 2:
        _compare(f"refused {_id(shape)} torch heads", shape, 1, heads, model, seed=300 + list(REFUSED).index(shape))


def test_a_search_with_the_largest_net_is_the_same_with_and_without_graph_capture():
    """(9,4,48,1) at gain 4 -- gate_columns<3>, one workgroup per CU -- inside BatchedMCTS: 256 trees, 20 simulations; visit
    counts, root priors and root values are equal whether the step-wise search is captured in a graph or not."""
    mcts_mod = _pkg("mcts")
    shape = (9, 4, 48, 1)
    model = lr.fresh_net(*shape, seed=48, gain=4)
    heads = model.heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipLstmHeads"
    n, sims = 256, 20
    obs = (torch.rand(n, shape[0], generator=torch.Generator().manual_seed(9)) - 0.5).cuda().contiguous()
    res = []
    for use_graph in (False, True):
        m = mcts_mod.BatchedMCTS(n, num_simulations=sims, maxium_action_sample=2, discount=0.999, root_exploration_fraction=0.1,
                                 use_graph=use_graph)
        for _ in range(2 if use_graph else 1):       # the second pass replays the captured graph
            m.seed(np.arange(n, dtype=np.uint64))
            eng = m.run(obs, heads, train=True)
        visits, priors, root_value, _ = eng.root_stats()
        torch.cuda.synchronize()
        assert m._single is None and (m._graph is not None) == use_graph
        res.append((visits.cpu().numpy().copy(), priors.cpu().numpy().copy(), root_value.cpu().numpy().copy()))
    (va, pa, ra), (vb, pb, rb) = res
    assert (va.sum(1) == sims).all() and np.isfinite(ra).all()
    assert np.array_equal(va, vb) and np.array_equal(pa, pb) and np.array_equal(ra, rb)
