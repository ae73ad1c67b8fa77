"""The large-action mlp_model head kernel (csrc/smz_mlp_large.hip: smz_mlp_recurrent_large through heads.HipMlpLargeHeads,
Muzero.heads(backend="large")) over the envelope smz_mlp_layout_large accepts, against the float64 restatement of
tests/mlp_reference.py.  Shapes are (obs, A, S, H, L); the kernel's panel width is 128, the width of wide_layer.

What each shape is the first to exercise:
  (1,1,1,1,0)        every dimension 1: one panel with one column, a one-row action table, S = 1 (span 0 + 1e-5)
  (3,2,5,7,2)        S = 5: the hidden part of the input layer ends inside an 8-input group; the mid layer applied twice
  (7,3,8,8,0)        S = 8: no padding inputs at all
  (4,100,29,64,0)    the smallest shape smz_mlp_layout_wide refuses on A + S; still one policy panel
  (4,128,8,16,1)     a policy panel filled exactly
  (4,129,8,16,1)     a second panel holding one column; the softmax across a panel boundary
  (4,362,32,64,1)    three panels, ragged last; 2 S = 64
  (4,1000,16,64,1)   the action count of the reference fixture la_A1000_K2_sims20: eight panels, ragged last
  (5,1024,64,128,4)  every limit at once; L = 4
Every case's action column holds A - 1, 0 and, where A allows, 127 and 128 (the last row of the first panel's part of the
table and the first of the second's), as far as the case has rows for them; the test asserts it on its inputs.

Tolerances are those of tests/test_gpu_mlp_envelope.py, taken from there: the bound of an output is max(contract, 4 x e32),
contract = TILE_ATOL (hidden rows 4e-6, policies 2e-6), e32 = the largest error of the float32 Restatement against the float64
one on the same rows, recomputed on the CPU in every run; decoded rewards and values within golden_util.DECODE_BOUND_STEPS
stairs (_decoded).  Rows at the + 1e-5 discontinuity of the scaling could be left out through _hidden_rows (at most 1 %), but
the net and input seeds are chosen so that the float64 restatement alone has no such row (0.5e-5 <= span <= 2e-5, S >= 2):
every case asserts that on the CPU before it touches the GPU, so the cap never does any work.

Measured on MI355X (profiles/mlp_large_heads_tolerances.jsonl is one run with SMZ_TOLERANCE_LOG set), worst over all cases of this
file: hidden rows 5.9e-7 ((5,1024,64,128,4) at gain 1; bound 4e-6), policies 5.6e-8 ((3,2,5,7,2) at gain 16; bound 2e-6), decoded rewards
0.772 and values 0.763 stairs ((5,1024,64,128,4) at gain 16; bound 1.05).  The contract bound was the active one in every case
(4 x e32 stayed below it: e32 at most 7.3e-7 on hidden rows, 5.6e-8 on policies), no stairs widening, no row left out.

Launch geometry (smz_mlp_recurrent_large; SMZ_MLP_LARGE_SPLIT_MAX must be unset).  Small batches run
k_mlp_recurrent_large_split: one workgroup of 4 wavefronts per chunk of 16 rows and branch, the tile's panels shared among the
wavefronts -- up to B = 2048 with one policy panel (A <= 128), up to B = 4096 with more.  Above that k_mlp_recurrent_large:
chunks of 32 rows on 4 wavefronts, a wavefront per tile, at most 2048 workgroups.  Every shape runs at B = 2048 (split), 4096
(split for A > 128) and 4097 (never split); (4,128,8,16,1) also at B = 2049 and (4,129,8,16,1) at 4096 / 4097 with one branch
only: both sides of both switches.  The searches of tests/test_gpu_large_heads_search.py run the split kernel at 8 to 128
trees.  Workgroup 0 of k_mlp_recurrent_large starts its second grid-stride trip at row 65 536: B = 65 553 runs it here, on the
small shape (4,129,8,16,1), with a ragged last chunk.  The split kernel never makes a second trip."""
import ctypes as C
import os
from importlib import import_module

import pytest
import torch

import mlp_reference as mr
from test_gpu_lstm import _FakeEngine, _held
from test_gpu_lstm_envelope import NAN_BITS, _decoded, _guarded, _hidden_rows, _untouched
from test_gpu_mlp_envelope import TILE_ATOL

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 0), (3, 2, 5, 7, 2), (7, 3, 8, 8, 0), (4, 100, 29, 64, 0), (4, 128, 8, 16, 1), (4, 129, 8, 16, 1),
          (4, 362, 32, 64, 1), (4, 1000, 16, 64, 1), (5, 1024, 64, 128, 4)]
GAINS = (1, 4, 16)
B = 4096
EDGE = (4, 129, 8, 16, 1)
ONE_PANEL = (4, 128, 8, 16, 1)
SPLIT_MAX = {False: 2048, True: 4096}   # the last batch of k_mlp_recurrent_large_split, by "A > 128" (smz_mlp_recurrent_large)
SECOND_TRIP = 2048 * 32 + 17           # the first row of workgroup 0's second trip is 65 536; a ragged last chunk


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _id(shape):
    return "x".join(str(v) for v in shape)


def _required_actions(A):
    return list(dict.fromkeys([A - 1, 0] + [a for a in (127, 128) if a < A]))


def _inputs(shape, seed, rows=B, branches="mixed"):
    _, A, S, _, _ = shape
    g = torch.Generator().manual_seed(seed)
    h = torch.rand(rows, S, generator=g)
    a = torch.randint(0, A, (rows,), generator=g)
    br = torch.randint(0, 2, (rows,), generator=g)
    need = _required_actions(A)[:rows]
    a[:len(need)] = torch.tensor(need)
    assert set(need) <= set(a.tolist()) and int(a.min()) >= 0 and int(a.max()) < A
    if branches != "mixed":
        br = torch.full_like(br, 1 if branches == "dyn" else 0)
    elif rows >= 64:
        assert 0.4 < float(br.float().mean()) < 0.6
    return h, a, br


def _case(shape, net_seed, gain, in_seed, rows=B, branches="mixed"):
    model = mr.fresh_net(*shape, seed=net_seed, gain=gain)
    h, a, br = _inputs(shape, in_seed, rows, branches)
    r64, r32 = mr.Restatement(model), mr.Restatement(model, torch.float32)
    out64 = r64.recurrent(h, a, br)
    if shape[2] >= 2:       # no row at the discontinuity of the scaling, by the float64 restatement alone
        assert not bool(((out64["span"] >= 0.5e-5) & (out64["span"] <= 2e-5)).any())
    return model, (h, a, br), out64, r32.recurrent(h, a, br)


def _engine_rows(h, a, br):
    fe = _FakeEngine()
    fe.parent_hidden = torch.as_tensor(h, dtype=torch.float32).cuda().contiguous()
    fe.last_action = torch.as_tensor(a).int().cuda()
    fe.branch = torch.as_tensor(br).to(torch.uint8).cuda()
    fe.B, fe.S = fe.parent_hidden.shape
    return fe


def _bounds(out64, out32):
    e32 = {k: float((out64[k] - out32[k].double()).abs().max()) for k in ("hidden", "policy")}
    return e32, {k: max(TILE_ATOL[k], 4 * e32[k]) for k in e32}


def _large(model):
    heads = model.heads("cuda:0", backend="large")
    assert type(heads).__name__ == "HipMlpLargeHeads" and heads.large_desc.A == model.action_dimension
    return heads


def _compare(tag, shape, gain, heads, case, rows=None):
    """`rows`: compare these rows only (a boolean mask); the bounds come from all rows of the case."""
    _, A, S, _, _ = shape
    _, (h, a, br), out64, out32 = case
    e32, bound = _bounds(out64, out32)
    print(f"{tag}: e32 " + ", ".join(f"{k} {v:.2e}" for k, v in e32.items()))
    h2, rw, p2, v2 = (t.clone().cpu() for t in heads.recurrent(_engine_rows(h, a, br)))
    assert h2.shape == (h.shape[0], S) and p2.shape == (h.shape[0], A)
    keep = _hidden_rows(out64["span"], S)
    assert bool(keep.all())
    sel = torch.ones_like(keep) if rows is None else rows
    if S == 1:      # span exactly 0 on both sides: (x - x) / 1e-5
        assert (h2 == 0).all() and (out64["hidden"] == 0).all()
    _held(f"{tag} hidden", h2[sel], out64["hidden"][sel], bound["hidden"])
    _held(f"{tag} policy", p2[sel], out64["policy"][sel], bound["policy"])
    assert (rw[br == 0] == 0).all()
    pick = lambda d: {k: v[sel] for k, v in d.items()}
    if bool(((br != 0) & sel).any()):
        _decoded(f"{tag} reward", rw[sel], pick(out64), pick(out32), "reward", gain, (br != 0)[sel])
    _decoded(f"{tag} value", v2[sel], pick(out64), pick(out32), "value", gain, torch.ones_like(br, dtype=torch.bool)[sel])
    return h2, rw, p2, v2


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_large_heads_match_the_float64_restatement(shape, gain):
    """4096 rows of mixed branches per shape and gain: k_mlp_recurrent_large (128 workgroups of 4 wavefronts) for the shapes
    with one policy panel, k_mlp_recurrent_large_split (2 x 256 workgroups) for those with more."""
    i = SHAPES.index(shape)
    case = _case(shape, 100 + i, gain, 7 + i)
    _compare(f"large {_id(shape)} gain {gain}", shape, gain, _large(case[0]), case)


@pytest.mark.parametrize("rows", [2048, 4097])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_large_heads_match_the_float64_restatement_in_either_geometry(shape, rows):
    """Gain 4.  B = 2048: k_mlp_recurrent_large_split for every shape (2 x 128 workgroups, four wavefronts per tile) -- one panel
    for wavefront 0 alone (A <= 128: the other three bring no maximum), panels % 4 from 1 to 0 and the value panel on each of
    the four wavefronts in turn (A = 1, 129, 362, 1000 / 1024: wavefronts 1, 2, 3, 0).  B = 4097: k_mlp_recurrent_large for every
    shape, the first batch that never splits."""
    assert "SMZ_MLP_LARGE_SPLIT_MAX" not in os.environ and (rows <= SPLIT_MAX[False] or rows > SPLIT_MAX[True])
    i = SHAPES.index(shape)
    case = _case(shape, 120 + i, 4, 27 + i + rows % 7, rows)
    _compare(f"large {_id(shape)} B {rows} gain 4", shape, 4, _large(case[0]), case)


@pytest.mark.parametrize("shape,rows,branches", [(EDGE, 4096, "dyn"), (EDGE, 4096, "ady"), (EDGE, 4097, "dyn"), (EDGE, 4097, "ady"),
                                                 (EDGE, 1, "mixed"), (EDGE, 16, "mixed"), (EDGE, 17, "mixed"),
                                                 (ONE_PANEL, 2049, "mixed"), (EDGE, SECOND_TRIP, "mixed")],
                         ids=["split_all_dynamics", "split_all_afterstate", "all_dynamics", "all_afterstate", "B1", "B16", "B17",
                              "one_panel_B2049", "second_grid_stride_trip"])
def test_large_heads_on_one_branch_ragged_batches_and_the_second_grid_stride_trip(shape, rows, branches):
    """Gain 4.  (4,129,8,16,1): batches of one branch only in either kernel, B = 4096 (the last split batch of a shape with two
    panels) and 4097 (no tile of the other branch: t0 or t1 is 0; the split kernel's workgroups of the other branch leave
    without a barrier); B = 1, 16 and 17 (ragged tiles, a second chunk of one row); B = 65 553: workgroup 0 of
    k_mlp_recurrent_large comes round a second time.  (4,128,8,16,1) at B = 2049: the first batch of a one-panel shape that does
    not split."""
    assert "SMZ_MLP_LARGE_SPLIT_MAX" not in os.environ
    assert (shape[1] > 128) == (shape == EDGE) and SPLIT_MAX[True] == B == 4096 and SPLIT_MAX[False] == 2048
    case = _case(shape, 140, 4, 47 + rows % 97, rows, branches)
    _compare(f"large {_id(shape)} B {rows} {branches} gain 4", shape, 4, _large(case[0]), case)


def _launch(heads, h, a, br, guard=True):
    """smz_mlp_recurrent_large through ctypes on the test's own guarded buffers -> the four outputs as int32 bit patterns."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    n, S, A = h.shape[0], heads.S, heads.A
    fe = _engine_rows(h, a, br)
    widths = dict(hidden=S, reward=1, policy=A, value=1)
    out = {k: _guarded(n, w) for k, w in widths.items()}
    p = lambda t: C.c_void_p(t.data_ptr())
    lib_mod.check(lib.smz_mlp_recurrent_large(C.byref(heads.large_desc), p(heads.packed), p(fe.parent_hidden), p(fe.last_action),
                                              p(fe.branch), p(out["hidden"]), p(out["reward"]), p(out["policy"]), p(out["value"]), n,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for k, w in widths.items():
        assert _untouched(out[k], n, w), (n, k)
        assert not bool((out[k][:n * w] == NAN_BITS).any()), (n, k)
    return {k: out[k][:n * w].cpu() for k, w in widths.items()}


@pytest.mark.parametrize("rows", [1, 17])
def test_nothing_is_written_beyond_the_rows_and_rows_do_not_depend_on_the_batch(rows):
    """(4,129,8,16,1), A = 129 (a last panel of one column), B = 1 and 17: the 8 guard rows behind row B - 1 of every output
    keep their NaN pattern -- nothing beyond [B, S], [B, A], [B] -- every element inside is written, and the rows are, bit for
    bit, those of a 64-row launch (whichever tile computed them)."""
    model = mr.fresh_net(*EDGE, seed=141, gain=4)
    heads = _large(model)
    h, a, br = _inputs(EDGE, 61, 64)
    want, got = _launch(heads, h, a, br), _launch(heads, h[:rows], a[:rows], br[:rows])
    for k, v in got.items():
        assert torch.equal(v, want[k][:v.numel()]), (rows, k)


def test_an_action_outside_the_table_is_evaluated_as_action_0():
    """(4,129,8,16,1), B = 64, once with valid actions and once with rows 1, 17 and 63 carrying last_action = A -- what the
    row of a tree that is switched off may hold (smz_select leaves it unwritten).  A is one past the table: a kernel that
    failed to range-check would read the next piece of the same weight allocation (asserted from the descriptor), never
    unmapped memory.  Every other row is bit-identical between the two runs; the three rows are the restatement's for
    action 0.  No other out-of-range value is used anywhere in the tests."""
    shape, rows, bad = EDGE, 64, [1, 17, 63]
    _, A, S, _, _ = shape
    case = _case(shape, 142, 4, 63, rows)
    model, (h, a, br), _, _ = case
    heads = _large(model)
    d = heads.large_desc
    r8 = (S + 7) & ~7
    for m in (0, 1):        # row A of either action table lies inside the image: the table is not its last piece
        assert d.off[m] + (r8 + A + 1) * 128 <= d.total_floats and d.off[m] + (r8 + A) * 128 == d.off[m + 1]
    a = a.clone()
    a[bad] = torch.tensor([5, 128, 77])                          # (valid actions other than 0 on the three rows)
    good = _launch(heads, h, a, br)
    a_bad, a_zero = a.clone(), a.clone()
    a_bad[bad], a_zero[bad] = A, 0
    got = _launch(heads, h, a_bad, br)
    others = torch.ones(rows, dtype=torch.bool)
    others[bad] = False
    for k, w in dict(hidden=S, reward=1, policy=A, value=1).items():
        assert torch.equal(got[k].view(rows, w)[others], good[k].view(rows, w)[others]), k
    assert not torch.equal(got["hidden"].view(rows, S)[~others], good["hidden"].view(rows, S)[~others])
    r64, r32 = mr.Restatement(model), mr.Restatement(model, torch.float32)
    zero_case = (model, (h, a_zero, br), r64.recurrent(h, a_zero, br), r32.recurrent(h, a_zero, br))
    h2, rw, p2, v2 = _compare("large untrusted action rows", shape, 4, _SameRows(heads, a_bad), zero_case, rows=~others)
    for k, t in dict(hidden=h2, reward=rw, policy=p2, value=v2).items():
        assert torch.equal(t.reshape(-1).view(torch.int32), got[k]), k


class _SameRows:
    """heads whose recurrent() runs with another action column than the case's (the out-of-range one)."""

    def __init__(self, heads, actions):
        self.heads, self.actions = heads, actions

    def recurrent(self, fe):
        fe.last_action = self.actions.int().cuda()
        return self.heads.recurrent(fe)


def test_refusals():
    """Muzero.heads(backend="large") raises ValueError outside the layout's limits; smz_mlp_recurrent_large says
    SMZ_ERR_INVALID for a null weight, input or output pointer, for B = 0 and for a descriptor whose total_floats is not its
    own layout's (nothing is launched in any of these calls)."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    with pytest.raises(ValueError):
        mr.fresh_net(4, 2, 65, 64, 0, seed=1).heads("cuda:0", backend="large")
    model = mr.fresh_net(*EDGE, seed=143, gain=1)
    heads = _large(model)
    h, a, br = _inputs(EDGE, 64, 8)
    fe = _engine_rows(h, a, br)
    outs = [torch.zeros(8 * w, device="cuda") for w in (heads.S, 1, heads.A, 1)]
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [C.byref(heads.large_desc), p(heads.packed), p(fe.parent_hidden), p(fe.last_action), p(fe.branch), *[p(t) for t in outs], 8,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    assert lib.smz_mlp_recurrent_large(*args) == 0
    for i in range(9):
        assert lib.smz_mlp_recurrent_large(*[None if j == i else x for j, x in enumerate(args)]) == lib_mod.SMZ_ERR_INVALID, i
    assert lib.smz_mlp_recurrent_large(*args[:9], 0, args[10]) == lib_mod.SMZ_ERR_INVALID
    d = lib_mod.MlpDesc.from_buffer_copy(heads.large_desc)
    d.total_floats += 128
    assert lib.smz_mlp_recurrent_large(C.byref(d), *args[1:]) == lib_mod.SMZ_ERR_INVALID
    wide = lib_mod.MlpDesc(4, 2, 8, 16, 1)
    assert lib.smz_mlp_layout_wide(C.byref(wide)) == 0
    assert lib.smz_mlp_recurrent_large(C.byref(wide), *args[1:]) == lib_mod.SMZ_ERR_INVALID
    torch.cuda.synchronize()


def test_auto_is_unchanged_and_the_large_heads_meet_the_bounds_on_the_same_net():
    """(4,256,16,64,1): heads("cuda:0") -- "auto", through Muzero.heads_backend -- still hands out FusedMlpHeads; both those
    torch heads and the "large" heads of the same net meet the bounds on the same 4096 rows."""
    shape = (4, 256, 16, 64, 1)
    case = _case(shape, 150, 4, 71)
    model, (h, a, br), _, _ = case
    auto = model.heads("cuda:0")
    assert type(auto).__name__ == "FusedMlpHeads" and type(model.heads("cuda:0", backend="auto")).__name__ == "FusedMlpHeads"
    _compare(f"large {_id(shape)} gain 4", shape, 4, _large(model), case)

    class _Torch:
        def recurrent(self, fe):
            fe.mlp_input = torch.cat([fe.parent_hidden, torch.nn.functional.one_hot(fe.last_action.long(), shape[1]).float()], 1)
            return auto.recurrent(fe)
    _compare(f"torch {_id(shape)} gain 4", shape, 4, _Torch(), case)
