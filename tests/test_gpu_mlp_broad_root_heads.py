"""The HIP root evaluation of the broad mlp_model heads (csrc/smz_mlp_broad_root.hip: smz_mlp_initial_broad through
heads.HipMlpBroadHeads / HipMlpBroadBf16Heads with hip_root=True, Muzero.heads(backend="broad" / "broad_bf16", hip_root=True)),
against the float64 restatement of tests/mlp_reference.py.  The helpers are those of tests/test_gpu_mlp_root_heads.py, imported.
Shapes are (obs, A, S, H, L).

What each shape is the first to exercise:
  (1,1,1,1,0)           every dimension 1; S = 1: hidden exactly 0 on both sides
  (3,2,5,7,2)           obs and S end inside an 8-input group; the mid layer applied twice
  (8,3,8,8,0)           no padding input anywhere
  (9,2,128,128,1)       every panel exactly full; a second obs group holding one input
  (4,129,130,131,2)     every width a panel plus 1 - 3 columns: the minimum / maximum of the scaling and the softmax both cross a
                        panel boundary
  (129,513,100,384,0)   three trunk panels (one wavefront idle per layer); five policy panels (wavefront 0 takes two); obs > 128
  (6,4,64,256,1)        a cell of the rate grid
  (1024,1024,256,512,4) every limit at once; the largest LDS request (64 KB + 32 KB)

Tolerances are those of tests/test_gpu_mlp_root_heads.py (its _references): the bound of an output is max(contract, 4 x e32),
contract = TILE_ATOL of tests/test_gpu_mlp_envelope.py (hidden rows 4e-6, policies 2e-6), e32 = the largest error of the float32
Restatement against the float64 one on the same rows, recomputed on the CPU in every run.  No row is left out: every case asserts
on the CPU, before it touches the GPU, that the float64 restatement alone has no root_span in [0.5e-5, 2e-5] (S >= 2).  The nets
are mlp_reference.fresh_net with the representation's parameters multiplied by the gain too; net seed 300 + i and input seed
41 + i for case i hold that assertion at gains 1, 4 and 16 (checked on the CPU when the seeds were chosen).  The bf16 heads keep
a float32 image for the root: their root must be the float32 heads' bit for bit.

Measured on MI355X (profiles/mlp_broad_root_tolerances.jsonl is one run with SMZ_TOLERANCE_LOG set), worst over all cases of this
file, the same for both backends: hidden rows 1.1e-6 ((1024,1024,256,512,4) at gain 1; bound 4e-6), policies under the contract
bound 5.0e-7 ((6,4,64,256,1) at gain 16; bound 2e-6), policy row sums within 2.0e-7 of 1 (bound 1e-6).  The contract bound was the
active one in every case but the policies of (1024,1024,256,512,4) at gain 16: there float32 itself is 1.4e-5 off (e32), the bound
was 4 x e32 = 5.7e-5 and the kernel measured 1.7e-5.  Elsewhere e32 was at most 7.0e-7 on hidden rows and 4.1e-7 on policies.  The
root outputs recorded in the searches: hidden 5.7e-7, policies 2.4e-8.  No row left out.

Launch geometry, the same at every batch size: a workgroup of four wavefronts per 16-row tile, the grid capped at 2048
workgroups, so row 32 768 starts the second grid-stride trip of workgroup 0: B = 2048 x 16 + 17 = 32 785 runs it, ragged at the
end."""
import ctypes as C

import numpy as np
import pytest
import torch

from search_helpers import _pkg
from test_gpu_large_actions import _streams_equal, _trees_equal
from test_gpu_large_heads_search import _Recording, _search, _Tape
from test_gpu_lstm_envelope import NAN_BITS, _guarded, _untouched
from test_gpu_mlp_root_heads import DISTINCT, GAINS, ROWS, _net, _obs, _references, _root_matches

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 0), (3, 2, 5, 7, 2), (8, 3, 8, 8, 0), (9, 2, 128, 128, 1), (4, 129, 130, 131, 2), (129, 513, 100, 384, 0),
          (6, 4, 64, 256, 1), (1024, 1024, 256, 512, 4)]
BACKENDS = ("broad", "broad_bf16")
CLASSES = dict(broad="HipMlpBroadHeads", broad_bf16="HipMlpBroadBf16Heads")
NET_SEED, OBS_SEED = 300, 41
EDGE = (4, 129, 130, 131, 2)
GRID_CAP = 2048                             # kBroadRootMaxWgs: a workgroup per tile
SECOND_TRIP = GRID_CAP * 16 + 17            # the first row of the second grid-stride trip, and a ragged last tile
# (shape, trees, simulations, K, large-action handle): the searches of tests/test_gpu_broad_heads_search.py
SEARCHES = [((4, 4, 70, 200, 1), 16, 20, 2, False), ((4, 129, 70, 200, 1), 8, 10, 3, True)]
SEARCH_IDS = ["per_lane_A4", "large_actions_A129"]
SEARCH_NET_SEED, SEARCH_OBS_SEED = 331, 8


def _id(shape):
    return "x".join(str(v) for v in shape)


def _root_heads(model, backend):
    heads = model.heads("cuda:0", backend=backend, hip_root=True)
    assert type(heads).__name__ == CLASSES[backend] and heads.single_launch is None
    assert heads.hip_root and "initial" in vars(heads)          # (the HIP root is bound on the instance)
    assert ("root_packed" in vars(heads)) == (backend == "broad_bf16")
    return heads


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_hip_root_matches_the_float64_restatement(shape, gain):
    """531 rows (33 full tiles and a ragged one) of randn observations per shape and gain, net seed 300 + i, input seed 41 + i;
    both backends, the bf16 heads' root bit for bit the float32 heads'."""
    i = SHAPES.index(shape)
    model = _net(shape, NET_SEED + i, gain)
    o = _obs(shape, OBS_SEED + i)
    assert o.shape[0] == ROWS
    root64, e32, bound = _references(model, o, shape[2])
    print(f"broad root {_id(shape)} gain {gain}: e32 " + ", ".join(f"{k} {v:.2e}" for k, v in e32.items()))
    od = o.cuda().contiguous()
    got = {}
    for backend in BACKENDS:
        heads = _root_heads(model, backend)
        hid, pol = (t.clone().cpu() for t in heads.initial(od))
        _root_matches(f"{backend} root {_id(shape)} gain {gain}", shape, hid, pol, root64, bound)
        got[backend] = (hid, pol)
    for a, b in zip(got["broad"], got["broad_bf16"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _launch(heads, o):
    """The entry point through ctypes on the test's own guarded buffers -> hidden and policy as int32 bit patterns [B, width]."""
    lib_mod = _pkg("_lib")
    lib = lib_mod.load()
    n = o.shape[0]
    widths = dict(hidden=heads.S, policy=heads.A)
    out = {k: _guarded(n, w) for k, w in widths.items()}
    p = lambda t: C.c_void_p(t.data_ptr())
    od = o.cuda().contiguous()
    lib_mod.check(lib.smz_mlp_initial_broad(C.byref(heads.broad_desc), p(heads.packed), p(od), p(out["hidden"]), p(out["policy"]), n,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for k, w in widths.items():
        assert _untouched(out[k], n, w), (n, k)
        assert not bool((out[k][:n * w] == NAN_BITS).any()), (n, k)
    return {k: out[k][:n * w].view(n, w).cpu() for k, w in widths.items()}


def test_rows_do_not_depend_on_the_batch_and_nothing_else_is_written():
    """(4,129,130,131,2), gain 4, net seed 360, input seed 81.  67 distinct observation rows, each evaluated in a batch of 1; then
    batches of 1, 16, 17 (a ragged second tile in a second workgroup), 64, 65 and 32 785 rows (the grid cap is 2048 workgroups of
    one tile each: 2048 x 16 + 17 rows run the second grid-stride trip, ragged at the end) whose row r is distinct row r % 67:
    every output row is, bit for bit, the batch-of-1 result of its observation, the 8 guard rows behind row B - 1 of either
    output keep their NaN pattern and every element inside is written."""
    model = _net(EDGE, 360, 4)
    heads = _root_heads(model, "broad")
    distinct = _obs(EDGE, 81, DISTINCT)
    root64, _, bound = _references(model, distinct, EDGE[2])
    ones = [_launch(heads, distinct[i:i + 1]) for i in range(DISTINCT)]
    want = {k: torch.cat([r[k] for r in ones], 0) for k in ("hidden", "policy")}
    assert len({tuple(r) for r in want["hidden"].tolist()}) == DISTINCT
    for rows in (1, 16, 17, 64, 65, SECOND_TRIP):
        idx = torch.arange(rows) % DISTINCT
        got = _launch(heads, distinct[idx])
        for k, v in got.items():
            assert torch.equal(v, want[k][idx]), (rows, k)
    _root_matches(f"broad root {_id(EDGE)} batch of 1", EDGE, want["hidden"].view(torch.float32), want["policy"].view(torch.float32),
                  root64, bound)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape,B,sims,K,large", SEARCHES, ids=SEARCH_IDS)
def test_searches_with_the_hip_root(shape, B, sims, K, large, backend, recwarn):
    """Step-wise searches on hip_root broad heads, gain 4, net seed 331 (A = 4) / 332 (A = 129), input seed 8: the captured graph
    (the root launch inside it) equals the eager run bit for bit; a second engine fed the recorded head outputs builds the same
    trees and leaves the same stream positions; the recorded root outputs meet the bounds of the restatement test; no
    single-launch search is attempted."""
    model = _net(shape, SEARCH_NET_SEED + int(large), 4)
    obs = (torch.rand(B, shape[0], generator=torch.Generator().manual_seed(SEARCH_OBS_SEED)) - 0.5).contiguous()
    root64, _, bound = _references(model, obs, shape[2])
    heads = _root_heads(model, backend)
    obs = obs.cuda()
    seeds = np.arange(B, dtype=np.uint64) + 5
    out, engines = [], []
    for use_graph in (True, False):
        mc = _pkg("mcts").BatchedMCTS(B, num_simulations=sims, maxium_action_sample=K, use_graph=use_graph)
        mc.seed(seeds)
        eng = mc.run(obs, heads, train=True)
        assert bool(eng.large_actions) == large and eng.A == shape[1] and (mc._graph is not None) == use_graph
        torch.cuda.synchronize()
        engines.append((mc, eng))
        v, p, rv, cr = (x.clone() for x in eng.root_stats())
        out.append((v, p, rv))
        assert int(v.sum()) == B * sims
    for x, y in zip(*out):
        assert torch.equal(x, y)
    _trees_equal(engines[0][1], engines[1][1], B)
    _streams_equal(engines[0][1], engines[1][1], B)
    assert torch.equal(engines[0][1].act(1.0)[0], engines[1][1].act(1.0)[0])
    rec = _Recording(heads)
    _, eng = _search(B, rec, obs, seeds, sims, K)
    assert len(rec.rounds) == sims
    assert torch.equal(eng.root_stats()[0], out[1][0]) and torch.equal(eng.root_stats()[2], out[1][2])
    _, again = _search(B, _Tape(rec), obs, seeds, sims, K)
    _trees_equal(eng, again, B)
    _streams_equal(eng, again, B)
    _root_matches(f"{backend} search A{shape[1]} root", shape, rec.root[0], rec.root[1], root64, bound)
    assert not [w for w in recwarn if "single-launch" in str(w.message)]


def test_defaults_are_unchanged_and_updated_weights_give_new_hip_root_heads():
    """(6,4,64,256,1), gain 4, net seed 390, input seed 91.  Without the flag heads("cuda:0", backend="broad" / "broad_bf16")
    return evaluators whose `initial` is FusedMlpHeads.initial and, for bf16, without a float32 image; one in-place update of the
    representation and the policy head gives new hip_root heads of either backend whose root outputs follow the updated net's
    restatement and differ from the old ones -- the float32 image and the bf16 heads' root_packed alike."""
    fused = _pkg("heads").FusedMlpHeads
    shape = (6, 4, 64, 256, 1)
    model = _net(shape, 390, 4)
    o = _obs(shape, 91, 64)
    root64, _, bound = _references(model, o, shape[2])
    od = o.cuda().contiguous()
    for backend in BACKENDS:
        plain = model.heads("cuda:0", backend=backend)
        assert type(plain).__name__ == CLASSES[backend] and not plain.hip_root
        assert plain.initial.__func__ is fused.initial and "initial" not in vars(plain) and "root_packed" not in vars(plain)
        assert model.heads("cuda:0", backend=backend, hip_root=False) is plain
        flagged = _root_heads(model, backend)
        assert flagged is not plain and model.heads("cuda:0", backend=backend, hip_root=True) is flagged
        _root_matches(f"torch root {backend}", shape, *(t.clone().cpu() for t in plain.initial(od)), root64, bound)
    old = {b: _root_heads(model, b) for b in BACKENDS}
    before = {b: [t.clone().cpu() for t in old[b].initial(od)] for b in BACKENDS}
    with torch.no_grad():
        [m for m in model.prediction_function.policy if isinstance(m, torch.nn.Linear)][-1].bias.add_(torch.linspace(-1, 1, shape[1]))
        next(model.representation_function.parameters()).add_(0.01)
    root64, _, bound = _references(model, o, shape[2])
    for backend in BACKENDS:
        new = _root_heads(model, backend)
        assert new is not old[backend]
        hid, pol = (t.clone().cpu() for t in new.initial(od))
        _root_matches(f"{backend} hip root after an in-place update", shape, hid, pol, root64, bound)
        assert not torch.equal(pol, before[backend][1]) and not torch.equal(hid, before[backend][0])
