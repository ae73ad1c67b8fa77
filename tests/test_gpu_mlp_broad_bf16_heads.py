"""The bf16 broad mlp_model head kernel (csrc/smz_mlp_broad_bf16.hip: smz_mlp_recurrent_broad_bf16 through
heads.HipMlpBroadBf16Heads, Muzero.heads(backend="broad_bf16")) over the envelope smz_mlp_layout_broad_bf16 accepts, against the
float64 ROUNDED restatement of tests/mlp_bf16_reference.py: the real compat_mlp modules with every Linear weight and every Linear
input rounded to bf16, everything else in float64 -- the arithmetic include/smz.h states as the kernel's contract.  Shapes are
(obs, A, S, H, L); every layer is a sequence of 128-column panels shared by the four wavefronts of a workgroup, a panel a
sequence of 32-input MFMA steps.

What each shape is the first to exercise:
  (1,1,1,1,0)         every dimension 1; span 0 (+ 1e-5); 31 padding inputs in every step
  (3,2,5,129,1)       K = 129: the fifth 32-input step of the mid and output layers holds one input; a second trunk panel of one column
  (4,2,33,32,0)       S = 33 is one input into a second step; H = 32 fills exactly one step
  (4,2,65,64,0)       the reward and the state columns in panels of their own on one trunk panel
  (4,3,129,130,2)     reward, state and value logits each cross a panel boundary (the dynamics output layer on all four
                      wavefronts); pre_in has K = 129; L = 2
  (4,2,100,384,0)     three trunk panels: the fourth wavefront has none; L = 0
  (4,129,8,256,1)     two trunk panels filled exactly; the action table is 256 wide; two policy panels
  (4,1000,16,200,1)   eight policy panels on a two-panel trunk
  (5,1024,256,512,4)  every limit at once
Every case's action column holds A - 1, 0 and, where A allows, 127 and 128, as far as the case has rows for them; the test
asserts it on its inputs.

Batches are the smallest at which the kernel can go wrong: B = 33 in either chunk geometry (chunks of 32: two chunks, the second
holding one row, so one of its two workgroups leaves at once; chunks of 16: three) at gain 4 and, in the default geometry, at
gains 1, 4 and 16; B = 64 of one branch only; B = 1 and 17 on guarded buffers; for (3,2,5,129,1) alone B = 4096 and 4097, the
two sides of the geometry switch of smz_mlp_recurrent_broad_bf16.  SMZ_MLP_BROAD_BF16_SMALL_MAX, read on every call, replaces
the 4096 (0: chunks of 32 rows always); _geometry sets it, the tests without it assert that it is unset.

Bound of an output: max(contract, 4 x e32r).  e32r is the largest error of the float32 rounded restatement against the float64
one on the same rows, recomputed on the CPU in every run: it contains the bf16 roundings that flip between float32 and float64
accumulation, and the kernel (another float32 summation order) flips others of the same size; 4 is the factor of the float32
head tests.  Decoded rewards and values are compared in stairs of the decode (golden_util.decode_steps), through the rule of
test_gpu_lstm_envelope._decoded: golden_util.DECODE_BOUND_STEPS, widened per row by the stairs that 4 x the largest logit error
of the float32 rounded restatement amounts to (_stairs_of) when that restatement's own decode leaves the bound -- at every gain
here, not only at 16, because a flipped bf16 rounding moves a logit by 2^-9 of an activation at any gain -- and never below their
contract, which is in stairs.  CONTRACT is twice the worst error of one recorded run of this file and
tests/test_gpu_broad_bf16_heads_search.py against the float64 rounded restatement (profiles/mlp_broad_bf16_tolerances.jsonl, written
with SMZ_TOLERANCE_LOG set), rounded up to one significant digit; the kernel is deterministic, so the margin covers other
seeds, not noise.  It is kept per gain: the errors grow with the spread of the logits, which the test sets through the gain, and
one contract over the whole file would be that of (5,1024,256,512,4) at gain 16 (policies 1e-2, values 2e5 stairs: there the
float32 rounded restatement itself is thousands of stairs from the float64 one) and would check nothing at gains 1 and 4; no
per-gain contract exceeds it.  MEASURED_WORST below quotes that run: hidden rows 7.2e-5 / 1.5e-3 / 1.5e-3, policies 1.4e-7 /
3.4e-5 / 4.7e-3, decoded rewards 0.74 / 4.7 / 199 stairs, decoded values 0.65 / 18.4 / 6.2e4 stairs at gains 1 / 4 / 16.

Rows at the + 1e-5 discontinuity of the scaling could be left out through _hidden_rows (at most 1 %), but the net and input
seeds are chosen so that the float64 rounded restatement alone has no such row (0.5e-5 <= span <= 2e-5, S >= 2): every case
asserts that on the CPU before it touches the GPU, so the cap never does any work."""
import ctypes as C
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as gu
import lstm_reference as lr
import mlp_bf16_reference as br16
import mlp_reference as mr
from test_gpu_lstm_envelope import NAN_BITS, _guarded, _hidden_rows, _stairs_of, _untouched
from test_gpu_mlp_large_heads import _SameRows, _engine_rows, _id, _inputs, _required_actions

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 0), (3, 2, 5, 129, 1), (4, 2, 33, 32, 0), (4, 2, 65, 64, 0), (4, 3, 129, 130, 2), (4, 2, 100, 384, 0),
          (4, 129, 8, 256, 1), (4, 1000, 16, 200, 1), (5, 1024, 256, 512, 4)]
GAINS = (1, 4, 16)
SWITCH = 4096                       # the last batch in chunks of 16 rows (smz_mlp_recurrent_broad_bf16)
RAGGED_K = (3, 2, 5, 129, 1)
TABLE = (4, 129, 8, 256, 1)
ENV = "SMZ_MLP_BROAD_BF16_SMALL_MAX"
# By gain (the spread of the logits, which the test chooses).  Hidden rows and policies: absolute; decoded rewards and values:
# stairs of the decode.  MEASURED_WORST: one run on MI355X of this file and tests/test_gpu_broad_bf16_heads_search.py (gain 4)
# against the float64 rounded restatement (profiles/mlp_broad_bf16_tolerances.jsonl); every figure but three is from
# (5,1024,256,512,4): gain 1 policy from (4,2,65,64,0) -- reward too -- gain 1 value from (4,2,33,32,0), gain 4 policy from
# (4,2,100,384,0).  CONTRACT = 2 x MEASURED_WORST rounded up to one significant digit; no contract exceeds the whole file's.
MEASURED_WORST = {1: dict(hidden=7.22e-5, policy=1.39e-7, reward=0.739, value=0.653),
                  4: dict(hidden=1.48e-3, policy=3.41e-5, reward=4.73, value=18.4),
                  16: dict(hidden=1.48e-3, policy=4.73e-3, reward=199.0, value=6.22e4)}
CONTRACT = {1: dict(hidden=2e-4, policy=3e-7, reward=2.0, value=2.0),
            4: dict(hidden=3e-3, policy=7e-5, reward=10.0, value=40.0),
            16: dict(hidden=3e-3, policy=1e-2, reward=400.0, value=2e5)}


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _bf16(model):
    heads = model.heads("cuda:0", backend="broad_bf16")
    assert type(heads).__name__ == "HipMlpBroadBf16Heads" and heads.broad_bf16_desc.A == model.action_dimension
    assert heads.single_launch is None
    return heads


@pytest.fixture(params=["chunks16", "chunks32"])
def _geometry(request, monkeypatch):
    """Every call of the test runs k_mlp_recurrent_broad_bf16<16> / <32>, whatever the batch size."""
    monkeypatch.setenv(ENV, "100000000" if request.param == "chunks16" else "0")
    return request.param


_CASES = {}


def _case(shape, net_seed, gain, in_seed, rows, branches="mixed"):
    """model, inputs, the float64 and the float32 rounded restatements' outputs: computed once, shared, never changed."""
    key = (shape, net_seed, gain, in_seed, rows, branches)
    if key not in _CASES:
        model = mr.fresh_net(*shape, seed=net_seed, gain=gain)
        h, a, br = _inputs(shape, in_seed, rows, branches)
        out64 = br16.RoundedRestatement(model).recurrent(h, a, br)
        if shape[2] >= 2:       # no row at the discontinuity of the scaling, by the float64 rounded restatement alone
            assert not bool(((out64["span"] >= 0.5e-5) & (out64["span"] <= 2e-5)).any())
        _CASES[key] = (model, (h, a, br), out64, br16.RoundedRestatement(model, torch.float32).recurrent(h, a, br))
    return _CASES[key]


def _holds_the_required_actions(shape, case, rows):
    need = _required_actions(shape[1])[:rows]
    assert set(need) <= set(case[1][1].tolist())


def _decoded_stairs(got, ref64, ref32, key, rows, contract):
    """-> (stairs from the float64 decode, bound in stairs) of the row nearest to its own bound, and the largest stairs."""
    want = ref64[key].numpy()
    steps = gu.decode_steps(got.cpu().numpy(), want)
    widen = np.zeros_like(steps)
    logits64, logits32 = ref64[key + "_logits"], ref32[key + "_logits"].double()
    floor = gu.decode_steps(lr.decode(logits32).numpy(), want)[rows.numpy()]
    if floor.size and floor.max() > gu.DECODE_BOUND_STEPS:
        widen = _stairs_of(logits64, 4 * float((logits64 - logits32).abs().max()))
    bound = np.maximum(contract, gu.DECODE_BOUND_STEPS + widen)
    steps = np.where(rows.numpy(), steps, 0.0)
    i = int(np.argmax(steps / bound))
    return float(steps[i]), float(bound[i]), float(steps.max())


def check_outputs(tag, S, gain, outputs, inputs, out64, out32, rows=None):
    """The four outputs of one recurrent call against the bounds of the module docstring.  `rows`: compare these rows only (a
    boolean mask); the bounds come from all rows.  Every figure is printed (and logged with SMZ_TOLERANCE_LOG) before any is
    asserted."""
    h, a, br = inputs
    h2, rw, p2, v2 = outputs
    keep = _hidden_rows(out64["span"], S)
    assert bool(keep.all())
    sel = torch.ones_like(keep) if rows is None else rows
    if S == 1:      # span exactly 0 on both sides: (x - x) / 1e-5
        assert (h2 == 0).all() and (out64["hidden"] == 0).all()
    assert (rw[br == 0] == 0).all()
    figures = []
    for key, got in (("hidden", h2), ("policy", p2)):
        e32r = float((out64[key] - out32[key].double()).abs().max())
        err = float((got.double()[sel] - out64[key][sel]).abs().max())
        figures.append(dict(what=f"{tag} {key}", max_abs=err, atol=max(CONTRACT[gain][key], 4 * e32r), e32r=e32r))
    for key, got, has in (("reward", rw, br != 0), ("value", v2, torch.ones_like(br, dtype=torch.bool))):
        if bool((has & sel).any()):
            steps, bound, worst = _decoded_stairs(got, out64, out32, key, has & sel, CONTRACT[gain][key])
            figures.append(dict(what=f"{tag} {key} stairs", max_abs=steps, atol=bound, worst_stairs=worst))
    log = os.environ.get("SMZ_TOLERANCE_LOG")
    for f in figures:
        print(json.dumps(f))
        if log:
            with open(log, "a") as fh:
                fh.write(json.dumps(f) + "\n")
    for f in figures:
        assert f["max_abs"] <= f["atol"], f


def _compare(tag, shape, gain, heads, case, rows=None):
    _, A, S, _, _ = shape
    _, (h, a, br), out64, out32 = case
    out = tuple(t.clone().cpu() for t in heads.recurrent(_engine_rows(h, a, br)))
    assert out[0].shape == (h.shape[0], S) and out[2].shape == (h.shape[0], A)
    check_outputs(tag, S, gain, out, (h, a, br), out64, out32, rows)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_bf16_heads_match_the_rounded_restatement_on_two_chunks(shape, _geometry):
    """Gain 4, B = 33 in either geometry: with chunks of 32 two chunks, the second holding one row; with chunks of 16 three."""
    i = SHAPES.index(shape)
    case = _case(shape, 320 + i, 4, 31 + i, 33)
    _holds_the_required_actions(shape, case, 33)
    _compare(f"broad_bf16 {_id(shape)} B 33 {_geometry} gain 4", shape, 4, _bf16(case[0]), case)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_bf16_heads_match_the_rounded_restatement_at_every_gain(shape, gain):
    """B = 33 in the default geometry (chunks of 16) at gains 1, 4 and 16."""
    assert ENV not in os.environ
    i = SHAPES.index(shape)
    case = _case(shape, 300 + i, gain, 11 + i, 33)
    _holds_the_required_actions(shape, case, 33)
    _compare(f"broad_bf16 {_id(shape)} B 33 gain {gain}", shape, gain, _bf16(case[0]), case)


@pytest.mark.parametrize("rows", [SWITCH, SWITCH + 1])
def test_bf16_heads_on_either_side_of_the_geometry_switch(rows):
    """(3,2,5,129,1), gain 4: B = 4096, the last batch in chunks of 16 rows, and 4097, the first in chunks of 32 (2 x 129
    workgroups, about half of them with two tiles, the last chunk holding one row)."""
    assert ENV not in os.environ
    case = _case(RAGGED_K, 360, 4, 41, rows)
    _holds_the_required_actions(RAGGED_K, case, rows)
    _compare(f"broad_bf16 {_id(RAGGED_K)} B {rows} gain 4", RAGGED_K, 4, _bf16(case[0]), case)


@pytest.mark.parametrize("branches", ["dyn", "ady"])
def test_bf16_heads_on_one_branch_only(branches, _geometry):
    """(3,2,5,129,1), gain 4, B = 64 of one branch, in either geometry: the workgroups of the other branch leave before the
    first barrier; with chunks of 32 every workgroup of the branch runs two full tiles."""
    case = _case(RAGGED_K, 340, 4, 51, 64, branches)
    assert len(set(case[1][2].tolist())) == 1
    _holds_the_required_actions(RAGGED_K, case, 64)
    _compare(f"broad_bf16 {_id(RAGGED_K)} B 64 {branches} {_geometry} gain 4", RAGGED_K, 4, _bf16(case[0]), case)


def _launch(heads, h, a, br):
    """smz_mlp_recurrent_broad_bf16 through ctypes on the test's own guarded buffers -> the four outputs as int32 bit patterns."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    n, S, A = h.shape[0], heads.S, heads.A
    fe = _engine_rows(h, a, br)
    widths = dict(hidden=S, reward=1, policy=A, value=1)
    out = {k: _guarded(n, w) for k, w in widths.items()}
    p = lambda t: C.c_void_p(t.data_ptr())
    lib_mod.check(lib.smz_mlp_recurrent_broad_bf16(C.byref(heads.broad_bf16_desc), p(heads.packed), p(fe.parent_hidden),
                                                   p(fe.last_action), p(fe.branch), p(out["hidden"]), p(out["reward"]),
                                                   p(out["policy"]), p(out["value"]), n,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for k, w in widths.items():
        assert _untouched(out[k], n, w), (n, k)
        assert not bool((out[k][:n * w] == NAN_BITS).any()), (n, k)
    return {k: out[k][:n * w].cpu() for k, w in widths.items()}


@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("shape", [RAGGED_K, TABLE], ids=_id)
def test_nothing_is_written_beyond_the_rows_and_rows_do_not_depend_on_the_batch(shape, rows, monkeypatch):
    """B = 1 and 17 on guarded buffers, in either geometry: the guard rows behind row B - 1 of every output keep their NaN
    pattern -- nothing beyond [B, S], [B, A], [B] -- every element inside is written, and the rows are, bit for bit, those of a
    64-row launch in chunks of 16 rows (whichever tile, and whichever place in it, computed them)."""
    model = mr.fresh_net(*shape, seed=341, gain=4)
    heads = _bf16(model)
    h, a, br = _inputs(shape, 61, 64)
    assert ENV not in os.environ
    want = _launch(heads, h, a, br)
    for small_max in ("100000000", "0"):
        monkeypatch.setenv(ENV, small_max)
        for n in (rows, 64):
            got = _launch(heads, h[:n], a[:n], br[:n])
            for k, v in got.items():
                assert torch.equal(v, want[k][:v.numel()]), (small_max, n, k)


@pytest.mark.parametrize("shape", [RAGGED_K, TABLE], ids=_id)
def test_an_action_outside_the_table_is_evaluated_as_action_0(shape):
    """B = 64, once with valid actions and once with rows 1, 17 and 63 carrying last_action = A.  A is one past the table: a
    kernel that failed to range-check would read the next piece of the same weight allocation (asserted from the descriptor),
    never unmapped memory.  Every other row is bit-identical between the two runs; the three rows are the rounded restatement's
    for action 0."""
    rows, bad = 64, [1, 17, 63]
    _, A, S, H, _ = shape
    model, (h, a, br), _, _ = _case(shape, 342, 4, 63, rows)
    heads = _bf16(model)
    d = heads.broad_bf16_desc
    r32, ph = (S + 31) & ~31, (H + 127) // 128
    for m in (0, 1):        # row A of either action table lies inside the image: the table is not its last piece
        assert d.off[m] + ph * (r32 + A + 1) * 64 <= d.total_floats and d.off[m] + ph * (r32 + A) * 64 == d.off[m + 1]
    a = a.clone()
    a[bad] = torch.tensor([1, A - 1, 1])                         # (valid actions other than 0 on the three rows)
    good = _launch(heads, h, a, br)
    a_bad, a_zero = a.clone(), a.clone()
    a_bad[bad], a_zero[bad] = A, 0
    got = _launch(heads, h, a_bad, br)
    others = torch.ones(rows, dtype=torch.bool)
    others[bad] = False
    for k, w in dict(hidden=S, reward=1, policy=A, value=1).items():
        assert torch.equal(got[k].view(rows, w)[others], good[k].view(rows, w)[others]), k
    assert not torch.equal(got["hidden"].view(rows, S)[~others], good["hidden"].view(rows, S)[~others])
    r64, r32r = br16.RoundedRestatement(model), br16.RoundedRestatement(model, torch.float32)
    zero_case = (model, (h, a_zero, br), r64.recurrent(h, a_zero, br), r32r.recurrent(h, a_zero, br))
    out = _compare(f"broad_bf16 {_id(shape)} untrusted action rows gain 4", shape, 4, _SameRows(heads, a_bad), zero_case, rows=~others)
    for k, t in zip(("hidden", "reward", "policy", "value"), out):
        assert torch.equal(t.reshape(-1).view(torch.int32), got[k]), k


def test_refusals():
    """Muzero.heads(backend="broad_bf16") raises ValueError outside the layout's limits; smz_mlp_recurrent_broad_bf16 says
    SMZ_ERR_INVALID for a null weight, input or output pointer, for B = 0 and B < 0, for a descriptor whose total_floats is not
    its own layout's, for one whose OP is not, and for the descriptors of the other three layouts -- the float32 broad layout of
    the same shape among them (nothing is launched in any of these calls)."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    for shape in [(4, 2, 8, 513, 0), (4, 2, 257, 64, 0), (4, 1025, 8, 16, 0)]:
        with pytest.raises(ValueError):
            mr.fresh_net(*shape, seed=1).heads("cuda:0", backend="broad_bf16")
    model = mr.fresh_net(*RAGGED_K, seed=343, gain=1)
    heads = _bf16(model)
    h, a, br = _inputs(RAGGED_K, 64, 8)
    fe = _engine_rows(h, a, br)
    outs = [torch.zeros(8 * w, device="cuda") for w in (heads.S, 1, heads.A, 1)]
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [C.byref(heads.broad_bf16_desc), p(heads.packed), p(fe.parent_hidden), p(fe.last_action), p(fe.branch), *[p(t) for t in outs],
            8, C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    entry = lib.smz_mlp_recurrent_broad_bf16
    assert entry(*args) == 0
    for i in range(9):
        assert entry(*[None if j == i else x for j, x in enumerate(args)]) == lib_mod.SMZ_ERR_INVALID, i
    for n in (0, -1):
        assert entry(*args[:9], n, args[10]) == lib_mod.SMZ_ERR_INVALID
    d = lib_mod.MlpDesc.from_buffer_copy(heads.broad_bf16_desc)
    d.total_floats += 128
    assert entry(C.byref(d), *args[1:]) == lib_mod.SMZ_ERR_INVALID
    d = lib_mod.MlpDesc.from_buffer_copy(heads.broad_bf16_desc)
    d.OP = 64
    assert entry(C.byref(d), *args[1:]) == lib_mod.SMZ_ERR_INVALID
    for layout, shape in (("smz_mlp_layout_wide", (4, 2, 8, 16, 1)), ("smz_mlp_layout_large", (4, 2, 8, 16, 1)),
                          ("smz_mlp_layout_broad", (4, 2, 8, 16, 1)), ("smz_mlp_layout_broad", RAGGED_K)):
        other = lib_mod.MlpDesc(*shape)
        assert getattr(lib, layout)(C.byref(other)) == 0
        assert entry(C.byref(other), *args[1:]) == lib_mod.SMZ_ERR_INVALID, layout
    # (and the float32 broad entry point refuses this layout's descriptor)
    assert lib.smz_mlp_recurrent_broad(*args) == lib_mod.SMZ_ERR_INVALID
    torch.cuda.synchronize()
