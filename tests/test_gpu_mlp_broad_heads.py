"""The broad mlp_model head kernel (csrc/smz_mlp_broad.hip: smz_mlp_recurrent_broad through heads.HipMlpBroadHeads,
Muzero.heads(backend="broad")) over the envelope smz_mlp_layout_broad accepts, against the float64 restatement of
tests/mlp_reference.py.  Shapes are (obs, A, S, H, L); every layer is a sequence of 128-column panels, shared by the four
wavefronts of a workgroup (wavefront w: panels w, w + 4, ...).

What each shape is the first to exercise:
  (1,1,1,1,0)         every dimension 1; span 0 (+ 1e-5)
  (3,2,5,129,1)       a second trunk panel of one column; the mid layer has K = 129: its last 8-input group is ragged
  (4,2,65,64,0)       2 S = 130 with one trunk panel: the reward and the state columns in panels of their own; the smallest
                      shape both older layouts refuse on S
  (4,3,129,130,2)     reward, state and value logits each cross a panel boundary (two panels each: the dynamics output layer
                      on all four wavefronts); pre_in has K = 129; L = 2
  (4,2,100,384,0)     three trunk panels: the fourth wavefront has none; L = 0
  (4,129,8,256,1)     two trunk panels filled exactly; the action table is 256 wide; two policy panels
  (4,1000,16,200,1)   eight policy panels on a two-panel trunk
  (5,1024,256,512,4)  every limit at once
Every case's action column holds A - 1, 0 and, where A allows, 127 and 128, as far as the case has rows for them; the test
asserts it on its inputs.

Tolerances: the rule of tests/test_gpu_mlp_large_heads.py, imported from there (_case, _compare): the bound of an output is
max(contract, 4 x e32), contract = TILE_ATOL (hidden rows 4e-6, policies 2e-6), e32 = the largest error of the float32
Restatement against the float64 one on the same rows, recomputed on the CPU in every run; decoded rewards and values within
golden_util.DECODE_BOUND_STEPS stairs (_decoded).  Rows at the + 1e-5 discontinuity of the scaling could be left out through
_hidden_rows (at most 1 %), but the net and input seeds are chosen so that the float64 restatement alone has no such row
(0.5e-5 <= span <= 2e-5, S >= 2): every case asserts that on the CPU before it touches the GPU, so the cap never does any work.

Measured on MI355X (profiles/mlp_broad_heads_tolerances.jsonl is one run with SMZ_TOLERANCE_LOG set), worst over all cases of
this file: hidden rows 1.3e-6 ((5,1024,256,512,4) at gain 1; bound 4e-6); policies 4.8e-7 ((4,2,100,384,0) at gain 16; bound 2e-6)
wherever the contract was the bound; decoded rewards 0.844 stairs ((4,2,100,384,0) at gain 16) and values 0.805
((4,3,129,130,2) at gain 16; bound 1.05).  The contract bound was the active one in every case but one, (5,1024,256,512,4) at
gain 16 and B = 4096: there the float32 restatement itself is 2.3e-5 off on policies (e32 on hidden rows at most 8.6e-7
anywhere), so 4 x e32 = 9.3e-5 was the policy bound (measured 3.1e-5), and the stairs widening of _decoded applied (the float32
logits alone move rows by more than the 1.05 stairs: the rows nearest to their own bounds were at 0.824 of 1.101 stairs, reward, and
0.889 of 1.061, value).  No row was left out anywhere.

Launch geometry (smz_mlp_recurrent_broad): workgroup (c, b) of four wavefronts takes the rows of branch b among the rows of
chunk c.  Up to B = 4096 a chunk is 16 rows -- at most one tile per workgroup -- above it is 32 rows, one or two tiles of 16 one
after the other (profiles/r16_broad_heads_chunk_ab.txt).  The environment variable SMZ_MLP_BROAD_SMALL_MAX, read on every call,
replaces the 4096 (0: chunks of 32 rows always); _geometry sets it so that every shape runs both kernels at B = 33 -- chunks of
32: two chunks, the second holding one row, so one of its two workgroups leaves at once; chunks of 16: three -- and the tests
without it assert that it is unset.  Every shape runs at B = 4096 (the last batch in chunks of 16) and, at gain 4, at B = 4097
(the first in chunks of 32, with a last chunk of one row).  One branch only: every workgroup of the other branch leaves at once."""
import ctypes as C
import os
from importlib import import_module

import pytest
import torch

import mlp_reference as mr
from test_gpu_lstm_envelope import NAN_BITS, _guarded, _untouched
from test_gpu_mlp_large_heads import _SameRows, _case, _compare, _engine_rows, _id, _inputs, _required_actions

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 0), (3, 2, 5, 129, 1), (4, 2, 65, 64, 0), (4, 3, 129, 130, 2), (4, 2, 100, 384, 0), (4, 129, 8, 256, 1),
          (4, 1000, 16, 200, 1), (5, 1024, 256, 512, 4)]
GAINS = (1, 4, 16)
B = 4096
RAGGED_K = (3, 2, 5, 129, 1)
TABLE = (4, 129, 8, 256, 1)


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _broad(model):
    heads = model.heads("cuda:0", backend="broad")
    assert type(heads).__name__ == "HipMlpBroadHeads" and heads.broad_desc.A == model.action_dimension
    assert heads.single_launch is None
    return heads


@pytest.fixture(params=["chunks16", "chunks32"])
def _geometry(request, monkeypatch):
    """Every call of the test runs k_mlp_recurrent_broad<16> / <32>, whatever the batch size."""
    monkeypatch.setenv("SMZ_MLP_BROAD_SMALL_MAX", "100000000" if request.param == "chunks16" else "0")
    return request.param


def _holds_the_required_actions(shape, case, rows):
    need = _required_actions(shape[1])[:rows]
    assert set(need) <= set(case[1][1].tolist())


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_broad_heads_match_the_float64_restatement(shape, gain):
    """4096 rows of mixed branches per shape and gain: 2 x 256 workgroups, a tile each."""
    assert "SMZ_MLP_BROAD_SMALL_MAX" not in os.environ
    i = SHAPES.index(shape)
    case = _case(shape, 200 + i, gain, 11 + i)
    _holds_the_required_actions(shape, case, B)
    _compare(f"broad {_id(shape)} gain {gain}", shape, gain, _broad(case[0]), case)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_broad_heads_match_the_float64_restatement_in_chunks_of_32(shape):
    """Gain 4, B = 4097: the first batch in chunks of 32 rows -- 2 x 129 workgroups, about half of them with two tiles, the last
    chunk holding one row."""
    assert "SMZ_MLP_BROAD_SMALL_MAX" not in os.environ
    i = SHAPES.index(shape)
    case = _case(shape, 260 + i, 4, 41 + i, 4097)
    _holds_the_required_actions(shape, case, 4097)
    _compare(f"broad {_id(shape)} B 4097 gain 4", shape, 4, _broad(case[0]), case)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_broad_heads_match_the_float64_restatement_on_two_chunks(shape, _geometry):
    """Gain 4, B = 33 in either geometry: with chunks of 32 two chunks, the second holding one row; with chunks of 16 three."""
    i = SHAPES.index(shape)
    case = _case(shape, 220 + i, 4, 31 + i, 33)
    _holds_the_required_actions(shape, case, 33)
    _compare(f"broad {_id(shape)} B 33 {_geometry} gain 4", shape, 4, _broad(case[0]), case)


@pytest.mark.parametrize("branches", ["dyn", "ady"])
def test_broad_heads_on_one_branch_only(branches, _geometry):
    """(3,2,5,129,1), gain 4, B = 64 of one branch, in either geometry: the workgroups of the other branch leave before the
    first barrier; with chunks of 32 every workgroup of the branch runs two full tiles."""
    case = _case(RAGGED_K, 240, 4, 51, 64, branches)
    assert len(set(case[1][2].tolist())) == 1
    _holds_the_required_actions(RAGGED_K, case, 64)
    _compare(f"broad {_id(RAGGED_K)} B 64 {branches} {_geometry} gain 4", RAGGED_K, 4, _broad(case[0]), case)


def _launch(heads, h, a, br):
    """smz_mlp_recurrent_broad through ctypes on the test's own guarded buffers -> the four outputs as int32 bit patterns."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    n, S, A = h.shape[0], heads.S, heads.A
    fe = _engine_rows(h, a, br)
    widths = dict(hidden=S, reward=1, policy=A, value=1)
    out = {k: _guarded(n, w) for k, w in widths.items()}
    p = lambda t: C.c_void_p(t.data_ptr())
    lib_mod.check(lib.smz_mlp_recurrent_broad(C.byref(heads.broad_desc), p(heads.packed), p(fe.parent_hidden), p(fe.last_action),
                                              p(fe.branch), p(out["hidden"]), p(out["reward"]), p(out["policy"]), p(out["value"]), n,
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
    model = mr.fresh_net(*shape, seed=241, gain=4)
    heads = _broad(model)
    h, a, br = _inputs(shape, 61, 64)
    assert "SMZ_MLP_BROAD_SMALL_MAX" not in os.environ
    want = _launch(heads, h, a, br)
    for small_max in ("100000000", "0"):
        monkeypatch.setenv("SMZ_MLP_BROAD_SMALL_MAX", small_max)
        for n in (rows, 64):
            got = _launch(heads, h[:n], a[:n], br[:n])
            for k, v in got.items():
                assert torch.equal(v, want[k][:v.numel()]), (small_max, n, k)


@pytest.mark.parametrize("shape", [RAGGED_K, TABLE], ids=_id)
def test_an_action_outside_the_table_is_evaluated_as_action_0(shape):
    """B = 64, once with valid actions and once with rows 1, 17 and 63 carrying last_action = A.  A is one past the table: a
    kernel that failed to range-check would read the next piece of the same weight allocation (asserted from the descriptor),
    never unmapped memory.  Every other row is bit-identical between the two runs; the three rows are the restatement's for
    action 0."""
    rows, bad = 64, [1, 17, 63]
    _, A, S, H, _ = shape
    case = _case(shape, 242, 4, 63, rows)
    model, (h, a, br), _, _ = case
    heads = _broad(model)
    d = heads.broad_desc
    r8, ph = (S + 7) & ~7, (H + 127) // 128
    for m in (0, 1):        # row A of either action table lies inside the image: the table is not its last piece
        assert d.off[m] + (ph * r8 + (A + 1) * ph) * 128 <= d.total_floats and d.off[m] + (ph * r8 + A * ph) * 128 == d.off[m + 1]
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
    r64, r32 = mr.Restatement(model), mr.Restatement(model, torch.float32)
    zero_case = (model, (h, a_zero, br), r64.recurrent(h, a_zero, br), r32.recurrent(h, a_zero, br))
    h2, rw, p2, v2 = _compare(f"broad {_id(shape)} untrusted action rows", shape, 4, _SameRows(heads, a_bad), zero_case, rows=~others)
    for k, t in dict(hidden=h2, reward=rw, policy=p2, value=v2).items():
        assert torch.equal(t.reshape(-1).view(torch.int32), got[k]), k


def test_refusals():
    """Muzero.heads(backend="broad") raises ValueError outside the layout's limits; smz_mlp_recurrent_broad says
    SMZ_ERR_INVALID for a null weight, input or output pointer, for B = 0 and B < 0, for a descriptor whose total_floats is not
    its own layout's, for one whose OP is not, and for the descriptors of the other two layouts (nothing is launched in any of
    these calls)."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    with pytest.raises(ValueError):
        mr.fresh_net(4, 2, 8, 513, 0, seed=1).heads("cuda:0", backend="broad")
    model = mr.fresh_net(*RAGGED_K, seed=243, gain=1)
    heads = _broad(model)
    h, a, br = _inputs(RAGGED_K, 64, 8)
    fe = _engine_rows(h, a, br)
    outs = [torch.zeros(8 * w, device="cuda") for w in (heads.S, 1, heads.A, 1)]
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [C.byref(heads.broad_desc), p(heads.packed), p(fe.parent_hidden), p(fe.last_action), p(fe.branch), *[p(t) for t in outs], 8,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    assert lib.smz_mlp_recurrent_broad(*args) == 0
    for i in range(9):
        assert lib.smz_mlp_recurrent_broad(*[None if j == i else x for j, x in enumerate(args)]) == lib_mod.SMZ_ERR_INVALID, i
    for n in (0, -1):
        assert lib.smz_mlp_recurrent_broad(*args[:9], n, args[10]) == lib_mod.SMZ_ERR_INVALID
    d = lib_mod.MlpDesc.from_buffer_copy(heads.broad_desc)
    d.total_floats += 128
    assert lib.smz_mlp_recurrent_broad(C.byref(d), *args[1:]) == lib_mod.SMZ_ERR_INVALID
    d = lib_mod.MlpDesc.from_buffer_copy(heads.broad_desc)
    d.OP = 64
    assert lib.smz_mlp_recurrent_broad(C.byref(d), *args[1:]) == lib_mod.SMZ_ERR_INVALID
    for layout in ("smz_mlp_layout_wide", "smz_mlp_layout_large"):
        other = lib_mod.MlpDesc(4, 2, 8, 16, 1)
        assert getattr(lib, layout)(C.byref(other)) == 0
        assert lib.smz_mlp_recurrent_broad(C.byref(other), *args[1:]) == lib_mod.SMZ_ERR_INVALID
    torch.cuda.synchronize()
