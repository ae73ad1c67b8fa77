"""Anchors tests/mlp_reference.py (the float64 restatement the GPU envelope test compares the HIP mlp_model kernels with) to
numbers the reference's own classes produced: every network call of the committed search tapes, evaluated as one batch.

Tolerances are those the GPU tests use for the same tapes (test_gpu_end_to_end.py): 1e-6 on hidden rows and policies
(test_batched_heads_match_reference_head_outputs); for the two wide checkpoints 2e-6 on hidden rows (cfg 434 shape), and 2e-6
on root hidden rows / 4e-6 on hidden rows / 2e-6 on policies (checkpoint 450, L 4).  The float32 restatement is the same
float32 modules the reference ran, batched instead of row by row; the float64 one must lie within the same bounds of the
reference's float32 numbers.  Observed (float32 / float64 restatement, worst of the six tapes): hidden rows
2.9e-7 (checkpoint 450) / 1.5e-7 (cfg 434 shape), policies 2.4e-7 / 1.0e-7 (both checkpoint 421).
Decoded rewards and values: the float32 restatement passes golden_util.assert_decoded_like_the_reference as it is; the
float64 decode is within golden_util.DECODE_BOUND_STEPS stairs of the reference's float32 decode, and "on the reference's
stair" -- which an exact value cannot be, it lies between two stairs of the float32 staircase -- is asked of the float64
logits rounded once to float32 and decoded in float32, the way the reference decodes (as in test_lstm_reference.py)."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as gu
import mlp_reference as mr
from lstm_reference import decode

# weights, tape, (root hidden, root policy, hidden, policy) tolerances of the GPU tests on the same tape
PAIRS = [("weights_ckpt421", "ckpt421_sims50", (1e-6, 1e-6, 1e-6, 1e-6)),
         ("weights_lunar_L0", "lunar_K2_sims50", (1e-6, 1e-6, 1e-6, 1e-6)),
         ("weights_lunar_L2", "lunarL2_K3_sims24", (1e-6, 1e-6, 1e-6, 1e-6)),
         ("weights_wide_A11", "wideA11_K9_sims24", (1e-6, 1e-6, 1e-6, 1e-6)),
         ("weights_ckpt450", "ckpt450_sims11", (2e-6, 1e-6, 4e-6, 2e-6)),
         ("weights_cfg434shape", "cfg434shape_sims11", (2e-6, 1e-6, 2e-6, 1e-6))]


def _model(wname):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd.model").Muzero.from_arrays(os.path.join(gu.GOLDEN, wname + ".npz"))


def _err(got, want):
    return float(np.abs(got.double().numpy() - np.asarray(want, np.float64)).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("wname,tape,tol", PAIRS, ids=[p[1] for p in PAIRS])
def test_restatement_reproduces_the_reference_tape(wname, tape, tol, dtype):
    ref = mr.Restatement(_model(wname), dtype)
    cfg, data = gu.load(tape)
    ncase, sims = data["tape_branch"].shape
    n = ncase * sims
    root = ref.initial(data["obs"])
    out = ref.recurrent(data["tape_hidden_in"].reshape(n, -1), data["tape_action"].reshape(-1), data["tape_branch"].reshape(-1))
    assert root["root_hidden"].dtype == dtype and out["hidden"].dtype == dtype and out["value"].dtype == dtype
    errs = (_err(root["root_hidden"], data["root_hidden"]), _err(root["root_policy"], data["root_policy"]),
            _err(out["hidden"], data["tape_hidden_out"].reshape(n, -1)), _err(out["policy"], data["tape_policy"].reshape(n, -1)))
    print(f"{tape} {dtype}: root hidden {errs[0]:.2e}, root policy {errs[1]:.2e}, hidden {errs[2]:.2e}, policy {errs[3]:.2e}")
    for what, e, t in zip(("root hidden", "root policy", "hidden", "policy"), errs, tol):
        assert e <= t, (what, e, t)
    dyn = torch.from_numpy(data["tape_branch"].reshape(-1) != 0)
    assert (out["reward"][~dyn] == 0).all() and (out["reward_logits"][~dyn] == 0).all()
    for what, logits, value, rec in (("reward", out["reward_logits"], out["reward"], data["tape_reward"]),
                                     ("value", out["value_logits"], out["value"], data["tape_value"])):
        if dtype == torch.float32:
            gu.assert_decoded_like_the_reference(value.numpy(), rec, what)
            continue
        assert gu.decode_steps(value.numpy(), rec.reshape(-1)).max() <= gu.DECODE_BOUND_STEPS, what
        as_the_reference = decode(logits.float())
        if what == "reward":
            as_the_reference = torch.where(dyn, as_the_reference, torch.zeros_like(as_the_reference))
        gu.assert_decoded_like_the_reference(as_the_reference.numpy(), rec, what)
    # no fixture row sits at the +1e-5 discontinuity of the scaling
    assert float(out["span"].min()) > 2e-5 and float(root["root_span"].min()) > 2e-5


def test_fresh_net_scales_the_recurrent_functions_only():
    a, b = mr.fresh_net(5, 3, 4, 6, 2, seed=3, gain=1), mr.fresh_net(5, 3, 4, 6, 2, seed=3, gain=4)
    for (ka, pa), (kb, pb) in zip(a.representation_function.state_dict().items(), b.representation_function.state_dict().items()):
        assert ka == kb and np.array_equal(pa.numpy(), pb.numpy())
    n = 0
    for f in ("prediction", "afterstate_prediction", "afterstate_dynamics", "dynamics"):
        for pa, pb in zip(getattr(a, f + "_function").parameters(), getattr(b, f + "_function").parameters()):
            assert np.array_equal(pa.detach().numpy() * np.float32(4), pb.detach().numpy())
            n += 1
    assert n == 4 * (2 + 2 + 2 * 2)          # per function: in (w, b) + the ONE shared mid (w, b) + two output heads (w, b)
    # the global generator is left where it was, and equal seeds give equal nets
    torch.manual_seed(11)
    want = torch.rand(3)
    torch.manual_seed(11)
    c = mr.fresh_net(5, 3, 4, 6, 2, seed=3, gain=1)
    assert torch.equal(torch.rand(3), want)
    assert all(torch.equal(x, y) for x, y in zip(a.dynamics_function.parameters(), c.dynamics_function.parameters()))


def test_restatement_does_not_alias_the_model():
    m = mr.fresh_net(4, 2, 5, 7, 1, seed=1, gain=1)
    ref = mr.Restatement(m)
    before = ref.initial(torch.zeros(2, 4))["root_policy"].clone()
    with torch.no_grad():
        for p in m.prediction_function.parameters():
            p.add_(1.0)
    assert torch.equal(ref.initial(torch.zeros(2, 4))["root_policy"], before)
    assert all(p.dtype == torch.float32 for p in m.prediction_function.parameters())
