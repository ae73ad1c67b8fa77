"""The HIP mlp_model head kernels (csrc/smz_mlp.hip, csrc/smz_mlp_device.hpp) over the whole envelope smz_mlp_layout and
smz_mlp_layout_wide accept, against the float64 restatement of tests/mlp_reference.py (anchored to the reference's own numbers
by tests/test_mlp_reference.py).  Shapes are (obs, A, S, H, L).

What each shape is there for (first shape that runs the path).
LDS-resident vector kernels k_mlp_initial / k_mlp_recurrent (HipMlpHeads):
  (1,1,1,1,0)      every dimension 1: dense() with one 4-input group; S = 1 -> span 0 (+ 1e-5), scaled state exactly 0; A = 1
  (1,1,1,1,3)      the same with the shared mid layer applied three times (L >= 3)
  (3,2,5,7,2)      H no multiple of 4 (the o < up4(H) zero padding of tA in trunk()); two groups: no unrolled body
  (6,5,12,17,1)    up4(H) = 20: five groups = unrolled body of 4 + tail of 1
  (4,2,28,63,0)    H = 63: 16 groups with one padded input; S even
  (4,3,31,64,0)    the FASTD instantiation k_mlp_recurrent<1, true> with A = 3 (never the matrix-core path)
  (4,32,32,64,0)   2 S = A + S = OP = 64: every lane in scale_lanes / decode_scale_lanes / softmax_decode_lanes
  (4,33,31,64,0)   A > 32 with A + S = 64
  (4,60,4,64,0)    A = 60: a policy over 60 lanes, S = 4
  (300,4,8,16,1)   an obs loop of 300 (75 groups = 72 + 3, longer than a wave); the scratch input sized by obs, not S + A
  (4,2,31,37,4)    L = 4; H = 37 -> 10 groups = 8 + 2
  (4,2,21,45,2)    nearest to the 160 KB budget (155,392 B); H = 45 -> 12 groups, no tail
Matrix-core tile kernel k_mlp_recurrent_mfma<2> / <4> (B = 8209 >= 8192: chunk 48, 172 workgroups, ragged last tiles):
  (4,2,31,64,0), (8,4,31,64,0), mixed branches, all dynamics (t1 = 0) and all afterstate (t0 = 0)
Wide tile kernel k_mlp_recurrent_wide (HipMlpTileHeads; K8 = 8-input groups of a layer, three prefetch slots per trip):
  (1,1,1,1,0)      K8 = 1 everywhere: only prefetch slot 0 is loaded
  (3,2,5,7,2)      K8x = K8h = K8s = 1 with the mid layers
  (7,3,8,8,0)      S = 8: 8 K8s - S = 0, the zero-fill loop must not run
  (4,2,14,20,1)    K8x = 2, K8h = 3: the second prefetch slot, one full trip of three
  (4,2,33,64,0)    the smallest shape the LDS layout refuses (what backend="auto" hands over); K8h = 8
  (4,100,28,100,2) A + S = 128, K8x = 16; H = 100 -> K8h = 13 = four trips + 1
  (4,2,64,65,1)    2 S = 128; S = 64 a multiple of 8
  (5,64,64,128,1)  every limit at once: H = 128, 2 S = 128, A + S = 128
  B = 8192 / 8193  the last batch with chunks of 32 rows on 4 waves / the first with chunks of 128 on 8 waves
Gains (mlp_reference.fresh_net): 1 = a fresh net (outputs ~1e-2), 4 and 16 spread the logits like a trained checkpoint's.

Tolerances.  Contract bounds: 1e-6 on hidden rows and policies for HipMlpHeads (test_batched_heads_match_reference_head_outputs),
4e-6 on hidden rows and 2e-6 on policies for HipMlpTileHeads (the checkpoint-450 test of test_gpu_end_to_end.py); decoded
rewards and values within golden_util.DECODE_BOUND_STEPS stairs of the float64 decode of the float64 logits.  The bound of an
output is max(contract, 4 x e32), e32 = the largest error of the float32 Restatement against the float64 one on the same rows,
computed here on the CPU: a property of the reference arithmetic, never of the kernels.  The factor 4 (that of
test_gpu_lstm_envelope.py) covers the kernels' legitimately different roundings -- the packed even / odd accumulation, the
MFMA chain, the hardware exp -- each of the order of e32; a wrong column, a dropped input group or a misplaced bias shows at
1e-3 and above.  On these nets and inputs e32 is largest on the hidden rows of (4,60,4,64,0) at gain 16 (S = 4, spans of 7e-3):
2.8e-6 on the host of the committed profile, 6.6e-6 on another CPU (torch's float32 GEMM sums in the order its vector width
gives); below 6.2e-7 on every other case, policies at most 1.8e-7, so the contract bound is the active one nearly everywhere.
These figures belong to the net and input seeds of this file; e32 is recomputed on every run and the `atol` of a logged line
is the bound that run used.  In the committed run that one case is the only one whose kernel error, 4.3e-6 = 1.5 e32 against
a bound of 1.12e-5, lies above its contract bound; every other hidden row and policy of every kernel is within 7.4e-7.  The
stairs widening of test_gpu_lstm_envelope._decoded applies at gain 16 only, and only where the float32 logits themselves leave
the bound.  Rows at the + 1e-5 discontinuity of the scaling (0.5e-5 <= span <= 2e-5) may be left out of the hidden comparison,
at most 1 % per case (_hidden_rows asserts it, and the share is logged); with these inputs none is: every logged share is 0
(smallest span for S >= 2: 6.2e-3).  For S = 1 the span and the scaled state are exactly 0 on both sides.

Known and deliberately not tested: the grid-stride second iteration of the tile kernels needs B > 256 x 2048 = 524,288 rows
for k_mlp_recurrent_mfma and B > 2048 x 2048 for k_mlp_recurrent_wide -- outside a seconds-long test.

With SMZ_TOLERANCE_LOG set, every comparison appends its largest error (profiles/mlp_envelope_tolerances.jsonl is one run)."""
import ctypes as C
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as gu
import mlp_reference as mr
from test_gpu_lstm import _FakeEngine, _engine_rows, _held  # noqa: F401
from test_gpu_lstm_envelope import NAN_BITS, _decoded, _guarded, _hidden_rows, _stairs_of, _untouched  # noqa: F401

pytestmark = pytest.mark.gpu

LDS_BUDGET = 160 * 1024
# (obs, A, S, H, L): LDS bytes of one smz_mlp_initial / smz_mlp_recurrent workgroup
SHAPES = {(1, 1, 1, 1, 0): 14464, (1, 1, 1, 1, 3): 19584, (3, 2, 5, 7, 2): 34304, (6, 5, 12, 17, 1): 75136,
          (4, 2, 28, 63, 0): 121472, (4, 3, 31, 64, 0): 125824, (4, 32, 32, 64, 0): 141056, (4, 33, 31, 64, 0): 141056,
          (4, 60, 4, 64, 0): 125824, (300, 4, 8, 16, 1): 142208, (4, 2, 31, 37, 4): 145536, (4, 2, 21, 45, 2): 155392}
MFMA_SHAPES = [(4, 2, 31, 64, 0), (8, 4, 31, 64, 0)]
MFMA_B = 8209
# shape: heads(backend="auto") hands out HipMlpTileHeads (else they are constructed directly: auto picks the LDS kernels)
WIDE_SHAPES = {(1, 1, 1, 1, 0): False, (3, 2, 5, 7, 2): False, (7, 3, 8, 8, 0): False, (4, 2, 14, 20, 1): False,
               (4, 2, 33, 64, 0): True, (4, 100, 28, 100, 2): True, (4, 2, 64, 65, 1): True, (5, 64, 64, 128, 1): True}
WIDE_SWITCH = [(4, 2, 33, 64, 0), (5, 64, 64, 128, 1)]
# refused by smz_mlp_layout: a layer wider than a wave (None) or weights + scratch beyond the budget (bytes)
REFUSED = {(4, 2, 33, 64, 0): None, (4, 2, 31, 65, 0): None, (4, 61, 4, 64, 0): None, (4, 2, 31, 64, 1): 207744,
           (4, 2, 31, 48, 2): 166272, (150, 2, 31, 64, 0): 167424}
REFUSED_WIDE = [(4, 2, 31, 129, 0), (4, 2, 65, 64, 0), (4, 100, 29, 64, 0)]
GAINS = (1, 4, 16)
B = 4096
LDS_ATOL = dict(hidden=1e-6, policy=1e-6)
TILE_ATOL = dict(hidden=4e-6, policy=2e-6)


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _up4(x):
    return (x + 3) & ~3


def _layout(shape, wide=False):
    lib_mod = _pkg("_lib")
    d = lib_mod.MlpDesc(*shape)
    lib = lib_mod.load()
    return (lib.smz_mlp_layout_wide if wide else lib.smz_mlp_layout)(C.byref(d)), d


def _lds_bytes(d):
    row_scratch = max(_up4(d.S + d.A), _up4(d.obs)) + _up4(d.H) + _up4(d.S)
    return (d.total_floats + 8 * row_scratch) * 4


def _id(shape):
    return "x".join(str(v) for v in shape)


def _inputs(shape, seed, rows=B, branches="mixed"):
    obs, A, S, _, _ = shape
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(rows, obs, generator=g) - 0.5
    h = torch.rand(rows, S, generator=g)
    a = torch.randint(0, A, (rows,), generator=g)
    br = torch.randint(0, 2, (rows,), generator=g)
    assert 0.4 < float(br.float().mean()) < 0.6
    if branches != "mixed":
        br = torch.full_like(br, 1 if branches == "dyn" else 0)
    return o, h, a, br


def _case(shape, net_seed, gain, in_seed, rows=B, branches="mixed"):
    """The net, its inputs and the float64 / float32 restatements on them (every test builds its own, once)."""
    model = mr.fresh_net(*shape, seed=net_seed, gain=gain)
    o, h, a, br = _inputs(shape, in_seed, rows, branches)
    r64, r32 = mr.Restatement(model), mr.Restatement(model, torch.float32)
    return model, (o, h, a, br), (r64.initial(o), r64.recurrent(h, a, br)), (r32.initial(o), r32.recurrent(h, a, br))


def _tile_heads(model, shape, by_auto):
    if by_auto:
        return model.heads("cuda:0")
    model_mod, heads_mod = _pkg("model"), _pkg("heads")
    arrays = model_mod.mlp_arrays_from_modules(model.representation_function, model.prediction_function,
                                               model.afterstate_prediction_function, model.afterstate_dynamics_function,
                                               model.dynamics_function)
    return heads_mod.HipMlpTileHeads(arrays, dict(zip(("obs", "A", "S", "H", "L"), shape)), "cuda:0")


def _compare(tag, shape, gain, heads, case, contract, root=True):
    _, A, S, _, _ = shape
    model, (o, h, a, br), (root64, out64), (root32, out32) = case
    e32 = {k: float((ref64[k] - ref32[k].double()).abs().max())
           for ref64, ref32, keys in ((root64, root32, ("root_hidden", "root_policy")), (out64, out32, ("hidden", "policy")))
           for k in keys}
    bound = {k: max(contract[k.replace("root_", "")], 4 * e32[k]) for k in e32}
    print(f"{tag}: e32 " + ", ".join(f"{k} {v:.2e}" for k, v in e32.items()))
    if root:
        hid, pol = (t.clone() for t in heads.initial(o.cuda().contiguous()))
    h2, rw, p2, v2 = (t.clone() for t in heads.recurrent(_engine_rows(h, a, br, A)))
    torch.cuda.synchronize()
    pairs = [("hidden", h2, out64, out64["span"])]
    if root:
        pairs.insert(0, ("root_hidden", hid, root64, root64["root_span"]))
    for key, got, ref, span in pairs:
        keep = _hidden_rows(span, S)                 # (asserts: at most 1 % of the rows left out; S = 1: every span 0)
        _held(f"{tag} {key} share of rows left out", [1.0 - float(keep.float().mean())], [0.0], 0.01)
        if S == 1:      # span exactly 0 on both sides: (x - x) / 1e-5
            assert (got.cpu() == 0).all() and (ref[key] == 0).all()
        _held(f"{tag} {key}", got.cpu()[keep], ref[key][keep], bound[key])
    if root:
        _held(f"{tag} root_policy", pol.cpu(), root64["root_policy"], bound["root_policy"])
    _held(f"{tag} policy", p2.cpu(), out64["policy"], bound["policy"])
    assert (rw.cpu()[br == 0] == 0).all()
    if bool((br != 0).any()):
        _decoded(f"{tag} reward", rw, out64, out32, "reward", gain, br != 0)
    _decoded(f"{tag} value", v2, out64, out32, "value", gain, torch.ones_like(br, dtype=torch.bool))


# ---- (a) the LDS-resident kernels ----------------------------------------------------------------------------------------

def test_every_shape_of_the_envelope_is_accepted_by_the_layout():
    assert len(SHAPES) == 12
    for shape, lds in SHAPES.items():
        rc, d = _layout(shape)
        assert rc == 0 and d.OP == 64 and _lds_bytes(d) == lds <= LDS_BUDGET, (shape, rc, d.OP, _lds_bytes(d))
    for shape in MFMA_SHAPES:
        rc, d = _layout(shape)
        assert rc == 0 and d.OP == 64 and _lds_bytes(d) <= LDS_BUDGET
    for shape in WIDE_SHAPES:
        rc, d = _layout(shape, wide=True)
        assert rc == 0 and d.OP == 128, (shape, rc)


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", list(SHAPES), ids=_id)
def test_hip_mlp_heads_match_the_float64_restatement(shape, gain):
    """4096 observations and 4096 recurrent rows of mixed branches per shape and gain (k_mlp_initial<1>, k_mlp_recurrent<1, false>;
    <1, true> at (4,3,31,64,0)).  Measured on MI355X (profiles/mlp_envelope_tolerances.jsonl), worst over the twelve shapes
    (gain 1 / 4 / 16): root hidden rows 4.7e-7 at every gain (at (4,33,31,64,0); the representation is not scaled by the gain), root
    policies 5.2e-8 / 5.6e-8 / 1.0e-7, hidden rows 5.3e-7 / 7.4e-7 / 4.3e-6 (all three at (4,60,4,64,0); bounds there 1e-6 /
    1.01e-6 / 1.12e-5 = 4 x e32; without that shape 4.5e-7 / 4.4e-7 / 4.2e-7), policies 5.2e-8 / 5.6e-8 / 1.1e-7; decoded rewards
    0.744 / 0.741 / 0.743 and values 0.747 / 0.749 / 0.751 stairs from the float64 decode, no case needed the stairs widening.
    The logged share of hidden rows left out at the + 1e-5 discontinuity of the scaling is 0 in every case (S = 1: span 0 and
    scaled state 0 on both sides)."""
    i = list(SHAPES).index(shape)
    case = _case(shape, 100 + i, gain, 7 + i)
    heads = case[0].heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipMlpHeads"
    _compare(f"lds {_id(shape)} gain {gain}", shape, gain, heads, case, LDS_ATOL)


@pytest.mark.parametrize("branches", ["mixed", "dyn", "ady"])
@pytest.mark.parametrize("shape", MFMA_SHAPES, ids=_id)
def test_matrix_core_heads_match_the_float64_restatement(shape, branches):
    """B = 8209 rows at gain 4: smz_mlp_recurrent takes k_mlp_recurrent_mfma<2> / <4> (B >= 8192, SMZ_MLP_MFMA_MIN unset):
    chunks of 48 rows on 172 workgroups, ragged last tiles; with one branch only, t0 or t1 is 0.  The root rows go through
    k_mlp_initial at rows_per_wave = 5.  Measured on MI355X, worst of the two shapes (mixed / all dynamics / all afterstate):
    hidden rows 5.4e-7 / 4.4e-7 / 5.4e-7 (bounds 1.02e-6 to 1.26e-6: 4 x e32 just above the contract), policies 5.4e-8 in all
    three, root hidden rows 5.3e-7, root policies 5.3e-8; rewards 0.741 and values 0.751 stairs; no row left out."""
    assert "SMZ_MLP_MFMA_MIN" not in os.environ and "SMZ_MLP_CHUNK" not in os.environ
    i = len(SHAPES) + MFMA_SHAPES.index(shape)
    case = _case(shape, 100 + i, 4, 7 + i, MFMA_B, branches)
    heads = case[0].heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipMlpHeads" and MFMA_B >= 8192
    _compare(f"mfma {_id(shape)} {branches} gain 4", shape, 4, heads, case, LDS_ATOL, root=branches == "mixed")


# ---- (b) the wide tile kernel ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", list(WIDE_SHAPES), ids=_id)
def test_hip_mlp_tile_heads_match_the_float64_restatement(shape, gain):
    """4096 rows of mixed branches through k_mlp_recurrent_wide (chunks of 32 rows, 4 waves); the root through the torch GEMMs
    of FusedMlpHeads.initial, which is what the search uses.  Measured on MI355X, worst over the eight shapes (gain 1 / 4 / 16):
    hidden rows 5.8e-7 / 5.2e-7 / 4.6e-7 (bound 4e-6), policies 5.3e-8 / 5.8e-8 / 1.6e-7 (bound 2e-6), root hidden rows 1.5e-7
    at every gain, root policies 5.3e-8 / 5.5e-8 / 1.4e-7; rewards 0.741 / 0.748 / 0.750 and values 0.723 / 0.748 / 0.762 stairs;
    the contract bound was the active one in every case, no stairs widening, no row left out."""
    i = list(WIDE_SHAPES).index(shape)
    case = _case(shape, 100 + i, gain, 7 + i)
    heads = _tile_heads(case[0], shape, WIDE_SHAPES[shape])
    assert type(heads).__name__ == "HipMlpTileHeads"
    _compare(f"wide {_id(shape)} gain {gain}", shape, gain, heads, case, TILE_ATOL)


@pytest.mark.parametrize("rows", [8192, 8193])
@pytest.mark.parametrize("shape", WIDE_SWITCH, ids=_id)
def test_hip_mlp_tile_heads_on_both_sides_of_the_geometry_switch(shape, rows):
    """Gain 4.  B = 8192: the last batch with chunks of 32 rows and 4 waves; B = 8193: the first with chunks of 128 and 8 waves.
    Measured on MI355X, worst of the four cases: hidden rows 5.5e-7, policies 5.8e-8, root hidden rows 1.4e-7, root policies
    5.4e-8, rewards 0.747 and values 0.746 stairs; no row left out."""
    i = list(WIDE_SHAPES).index(shape)
    case = _case(shape, 100 + i, 4, 7 + i, rows)
    heads = case[0].heads("cuda:0")
    assert type(heads).__name__ == "HipMlpTileHeads"
    _compare(f"wide {_id(shape)} B {rows} gain 4", shape, 4, heads, case, TILE_ATOL)


# ---- (d) rows do not depend on the launch geometry, and nothing else is written ----------------------------------------------

def _rows_input(shape, rows, seed):
    obs, A, S, _, _ = shape
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(rows, obs, generator=g) - 0.5).cuda()
    x = torch.cat([torch.rand(rows, S, generator=g), torch.nn.functional.one_hot(torch.randint(0, A, (rows,), generator=g), A).float()],
                  1).cuda()
    br = torch.randint(0, 2, (rows,), generator=g).to(torch.uint8).cuda()
    return o, x, br


def _launcher(shape, desc, weights, recurrent, initial, o_all, x_all, br_all):
    """launch(n, with_reward) -> the outputs of the first n rows as int32 bit patterns; asserts the 8 guard rows behind row
    n - 1 of every output (and the whole reward buffer of a call without one) keep their NaN pattern."""
    lib_mod = _pkg("_lib")
    _, A, S, _, _ = shape
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    widths = dict(hidden=S, reward=1, policy=A, value=1)
    if initial is not None:
        widths.update(root_hidden=S, root_policy=A)

    def launch(n, with_reward=True):
        o, x, br = o_all[:n].clone(), x_all[:n].clone(), br_all[:n].clone()
        out = {k: _guarded(n, w) for k, w in widths.items()}
        if initial is not None:
            lib_mod.check(initial(C.byref(desc), p(weights), p(o), p(out["root_hidden"]), p(out["root_policy"]), n, stream))
        lib_mod.check(recurrent(C.byref(desc), p(weights), p(x), p(br), p(out["hidden"]), p(out["reward"]) if with_reward else None,
                                p(out["policy"]), p(out["value"]), n, stream))
        torch.cuda.synchronize()
        for k, w in widths.items():
            assert _untouched(out[k], n if (with_reward or k != "reward") else 0, w), (n, k)
        return {k: out[k][:n * w].cpu() for k, w in widths.items()}
    return launch


def _same_rows(launch, big, smaller, without_reward):
    want = launch(big)
    assert not any(bool((v == NAN_BITS).any()) for v in want.values())
    assert torch.isfinite(want["hidden"].view(torch.float32)).all() and torch.isfinite(want["value"].view(torch.float32)).all()
    for n in smaller:
        for k, v in launch(n).items():
            assert torch.equal(v, want[k][:v.numel()]), (n, k)
    got = launch(without_reward, with_reward=False)
    for k in got:
        if k != "reward":
            assert torch.equal(got[k], want[k][:got[k].numel()]), k
    return want


def test_lds_kernel_rows_do_not_depend_on_the_launch_geometry_and_nothing_else_is_written():
    """smz_mlp_initial / smz_mlp_recurrent through ctypes on the test's own buffers, shape (4,2,21,45,2) at gain 4, B on both
    sides of every change of rows_per_wave (2048 waves: 1 row up to 2048, 2 up to 4096, then 3): the 8 guard rows behind row
    B - 1 of every output keep their NaN pattern, rows < B are bit for bit those of the B = 4097 launch (whichever wave
    computed them), and a call without a reward buffer leaves the other three outputs bit for bit the same."""
    lib = _pkg("_lib").load()
    shape = (4, 2, 21, 45, 2)
    heads = mr.fresh_net(*shape, seed=31, gain=4).heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipMlpHeads"
    launch = _launcher(shape, heads.desc, heads.weights, lib.smz_mlp_recurrent, lib.smz_mlp_initial, *_rows_input(shape, 4097, 77))
    _same_rows(launch, 4097, (1, 3, 5, 2047, 2048, 2049), 2049)


def test_wide_kernel_rows_do_not_depend_on_the_launch_geometry_and_nothing_else_is_written():
    """smz_mlp_recurrent_wide, shape (4,2,33,64,0) at gain 4: B = 1, 15, 16, 17, 33 and 8192 (chunks of 32 rows, 4 waves) against
    the rows of B = 8193 (chunks of 128, 8 waves) bit for bit, guards untouched, a call without a reward buffer; and two
    identical launches give identical bits -- the tile lists are filled with LDS atomics in arbitrary order, a leaf must not
    depend on its tile mates."""
    lib = _pkg("_lib").load()
    shape = (4, 2, 33, 64, 0)
    heads = mr.fresh_net(*shape, seed=33, gain=4).heads("cuda:0")
    assert type(heads).__name__ == "HipMlpTileHeads"
    launch = _launcher(shape, heads.wide_desc, heads.packed, lib.smz_mlp_recurrent_wide, None, *_rows_input(shape, 8193, 78))
    want = _same_rows(launch, 8193, (1, 15, 16, 17, 33, 8192), 8192)
    again = launch(8193)
    for k, v in again.items():
        assert torch.equal(v, want[k]), k


def test_matrix_core_kernel_writes_nothing_else_and_repeats_itself():
    """smz_mlp_recurrent on the matrix-core path, shape (4,2,31,64,0) at gain 4, B = 8209: guards untouched (a ragged tile
    repeats its first row and must not store for the repeats), two launches identical bit for bit, and a call without a
    reward buffer leaves the other outputs the same."""
    assert "SMZ_MLP_MFMA_MIN" not in os.environ and "SMZ_MLP_CHUNK" not in os.environ
    lib = _pkg("_lib").load()
    shape = (4, 2, 31, 64, 0)
    heads = mr.fresh_net(*shape, seed=35, gain=4).heads("cuda:0", backend="hip")
    launch = _launcher(shape, heads.desc, heads.weights, lib.smz_mlp_recurrent, None, *_rows_input(shape, MFMA_B, 79))
    _same_rows(launch, MFMA_B, (MFMA_B,), MFMA_B)


# ---- (e) refusals and routing ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(REFUSED), ids=_id)
def test_shapes_outside_the_lds_envelope_are_refused_and_routed_to_the_tile_heads(shape):
    """smz_mlp_layout says SMZ_ERR_INVALID, heads(backend="hip") raises, heads(backend="auto") hands out HipMlpTileHeads."""
    lib_mod = _pkg("_lib")
    rc, d = _layout(shape)
    assert rc == lib_mod.SMZ_ERR_INVALID
    if REFUSED[shape] is None:
        assert d.OP > 64
    else:
        assert d.OP == 64 and _lds_bytes(d) == REFUSED[shape] > LDS_BUDGET
    model = mr.fresh_net(*shape, seed=200 + list(REFUSED).index(shape), gain=1)
    with pytest.raises(ValueError):
        model.heads("cuda:0", backend="hip")
    assert type(model.heads("cuda:0", backend="auto")).__name__ == "HipMlpTileHeads"


@pytest.mark.parametrize("shape", REFUSED_WIDE, ids=_id)
def test_shapes_outside_the_wide_envelope_are_refused_and_fall_back_to_the_torch_heads(shape):
    """smz_mlp_layout_wide says SMZ_ERR_TOO_LARGE (H, 2 S or A + S beyond 128), constructing HipMlpTileHeads raises,
    heads(backend="auto") hands out FusedMlpHeads; for (4,2,31,129,0) those torch heads meet the tile heads' bounds against
    the restatement at gain 1 (measured: hidden rows 2.6e-7, policies 5.2e-8, decoded scalars 0.745 stairs)."""
    lib_mod = _pkg("_lib")
    assert _layout(shape, wide=True)[0] == lib_mod.SMZ_ERR_TOO_LARGE
    assert _layout(shape)[0] == lib_mod.SMZ_ERR_INVALID
    i = REFUSED_WIDE.index(shape)
    case = _case(shape, 300 + i, 1, 400 + i) if i == 0 else None
    model = case[0] if case else mr.fresh_net(*shape, seed=300 + i, gain=1)
    with pytest.raises(ValueError):
        model.heads("cuda:0", backend="hip")
    with pytest.raises(ValueError):
        _tile_heads(model, shape, False)
    heads = model.heads("cuda:0", backend="auto")
    assert type(heads).__name__ == "FusedMlpHeads"
    if case:
        _compare(f"refused {_id(shape)} torch heads", shape, 1, heads, case, TILE_ATOL)


# ---- (f) the paired tails inside the single-launch search ------------------------------------------------------------------

@pytest.mark.parametrize("tpw", [None, "2"], ids=["default_geometry", "two_trees_per_wave"])
@pytest.mark.parametrize("shape", [(4, 17, 16, 32, 0), (4, 1, 32, 64, 0), (4, 3, 31, 64, 0), (4, 2, 1, 8, 1), (4, 2, 9, 16, 1)],
                         ids=_id)
def test_single_launch_search_equals_stepwise_search_on_fresh_shapes(shape, tpw, monkeypatch):
    """smz_search_mlp (whole search in one kernel) against the step-wise kernels with the same HipMlpHeads, fresh nets at gain 4,
    130 trees x 12 simulations, K = 2, two consecutive searches: visits, float64 priors, root values, act(1.0) outputs, three
    dumped trees and the stream states bit for bit, as test_single_launch_search_equals_stepwise_search does for the shipped nets.
    (4,17,16,32,0) and (4,1,32,64,0): A + S == 33 with A != 2 (the one-output Q part of softmax_decode_pair); (4,3,31,64,0): the
    shipped dimensions on the generic instantiation (half_sum5); (4,2,1,8,1): S = 1; (4,2,9,16,1): the constructor's default S.
    The two-row pass recurrent_rows<1, 2, SAME> and its paired tails run when a wavefront owns two trees: 130 trees get one tree
    per wave by default (recurrent_rows<1, 1>), so each shape also runs with SMZ_SEARCH_TPW=2, the geometry of 4096 trees.
    With two trees per wave and S < 16, (4,2,1,8,1) and (4,2,9,16,1) guard dynamics_tail_pair's next-state lanes: outputs
    [S, 2 S) end inside the lower half-wave there, and the lanes behind output 2 S - 1 must neither enter the row's min / max
    nor be stored behind it.  No shape is refused with SMZ_ERR_TOO_LARGE: the step-wise fallback (m._single False, with a
    warning) would fail the assertion below."""
    mcts_mod = _pkg("mcts")
    if tpw is None:
        monkeypatch.delenv("SMZ_SEARCH_TPW", raising=False)
    else:
        monkeypatch.setenv("SMZ_SEARCH_TPW", tpw)
    model = mr.fresh_net(*shape, seed=500 + shape[1], gain=4)
    heads = model.heads("cuda:0", backend="hip")
    assert type(heads).__name__ == "HipMlpHeads"
    n, sims = 130, 12
    obs = (torch.rand(n, shape[0], generator=torch.Generator().manual_seed(1)) - 0.5).cuda().contiguous()
    res = []
    for single in (True, False):
        m = mcts_mod.BatchedMCTS(n, num_simulations=sims, maxium_action_sample=2, discount=0.997, root_exploration_fraction=0.25,
                                 use_graph=False, single_launch=single)
        m.seed(np.arange(n, dtype=np.uint64) + 5)
        for _ in range(2):
            e = m.run(obs, heads, train=True)
        assert m._single is (True if single else None)       # (False: the step-wise fallback after SMZ_ERR_TOO_LARGE)
        visits, priors, rv, cr = e.root_stats()
        action, policy, cv, _ = e.act(1.0)
        torch.cuda.synchronize()
        assert priors.dtype == torch.float64
        out = [t.cpu().numpy().copy() for t in (visits, priors, rv, cr, action, policy, cv)]
        res.append((out, [e.dump_tree(i) for i in (0, n // 2, n - 1)], [e.get_rng_state(i) for i in (0, 1, n - 1)]))
    assert (res[0][0][0].sum(1) == sims).all() and np.isfinite(res[0][0][2]).all()
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    for da, db in zip(res[0][1], res[1][1]):
        for k in da:
            assert np.array_equal(np.asarray(da[k]), np.asarray(db[k])), k
    for (ka, pa), (kb, pb) in zip(res[0][2], res[1][2]):
        assert np.array_equal(ka, kb) and pa == pb
