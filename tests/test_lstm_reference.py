"""Anchors tests/lstm_reference.py (the float64 restatement the GPU envelope test compares the HIP kernels with) to numbers
the reference's own classes produced: every network call of the search fixtures in tests/golden/lstm/ (tools/gen_golden_lstm.py).

Float64 against the reference's float32 results of the same modules: TOL of test_lstm_family.py (1e-6; observed 2.5e-7 on
hidden rows, 5.6e-8 on policies).  Decoded rewards and values: the float64 decode is within golden_util.DECODE_BOUND_STEPS
stairs of the reference's float32 decode (observed 0.71); golden_util.assert_decoded_like_the_reference, whose 60 % share "on
the reference's stair" an exact value cannot meet (it lies between two stairs of the float32 staircase), is applied to the
float64 logits rounded once to float32 and decoded in float32, the way the reference decodes."""
import numpy as np
import pytest
import torch

import golden_util as gu
import lstm_reference as lr
from test_lstm_family import NETS, TOL, _net


@pytest.mark.parametrize("name", sorted(NETS))
def test_float64_restatement_reproduces_the_reference_tape(name):
    ref = lr.Restatement(_net(name))
    cfg, data = gu.load("lstm/" + NETS[name])
    ncase, sims = data["tape_branch"].shape
    root = ref.initial(data["obs"])
    np.testing.assert_allclose(root["root_hidden"].numpy(), data["root_hidden"], atol=TOL, rtol=0)
    np.testing.assert_allclose(root["root_policy"].numpy(), data["root_policy"], atol=TOL, rtol=0)
    out = ref.recurrent(data["tape_hidden_in"].reshape(ncase * sims, -1), data["tape_action"].reshape(-1),
                        data["tape_branch"].reshape(-1))
    np.testing.assert_allclose(out["hidden"].numpy(), data["tape_hidden_out"].reshape(ncase * sims, -1), atol=TOL, rtol=0)
    np.testing.assert_allclose(out["policy"].numpy(), data["tape_policy"].reshape(ncase * sims, -1), atol=TOL, rtol=0)
    dyn = torch.from_numpy(data["tape_branch"].reshape(-1) != 0)
    assert (out["reward"][~dyn] == 0).all() and (out["reward_logits"][~dyn] == 0).all()
    # The reference's float32 decode is a staircase (golden_util.DECODE_STEP) and the exact value of the formula lies between two
    # stairs: the float64 decode is held to the bound of any float32 evaluation, and "on the reference's stair" is asked of the
    # float64 logits rounded once and decoded the way the reference decodes them, in float32.
    for what, logits, value, tape in (("reward", out["reward_logits"], out["reward"], data["tape_reward"]),
                                      ("value", out["value_logits"], out["value"], data["tape_value"])):
        assert gu.decode_steps(value.numpy(), tape.reshape(-1)).max() <= gu.DECODE_BOUND_STEPS, what
        as_the_reference = lr.decode(logits.float())
        if what == "reward":
            as_the_reference = torch.where(dyn, as_the_reference, torch.zeros_like(as_the_reference))
        gu.assert_decoded_like_the_reference(as_the_reference.numpy(), tape, what)
    assert float(out["span"].min()) > 2e-5          # no fixture row sits at the +1e-5 discontinuity of the scaling


def test_fresh_net_scales_the_recurrent_functions_only():
    a, b = lr.fresh_net(5, 3, 4, 2, seed=3, gain=1), lr.fresh_net(5, 3, 4, 2, seed=3, gain=4)
    for (ka, pa), (kb, pb) in zip(a.representation_function.state_dict().items(), b.representation_function.state_dict().items()):
        assert ka == kb and np.array_equal(pa.numpy(), pb.numpy())
    n = 0
    for f in ("prediction", "afterstate_prediction", "afterstate_dynamics", "dynamics"):
        for pa, pb in zip(getattr(a, f + "_function").parameters(), getattr(b, f + "_function").parameters()):
            assert np.array_equal(pa.detach().numpy() * np.float32(4), pb.detach().numpy())
            n += 1
    assert n == 7 * (2 + 4 * 2)          # seven trunks: Linear (w, b) + two LSTM layers (w_ih, w_hh, b_ih, b_hh)
