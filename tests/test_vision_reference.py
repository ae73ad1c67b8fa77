"""tests/vision_reference.py on the CPU: the staged restatement the GPU envelope test (tests/test_gpu_vision_envelope.py) judges
the HIP vision heads by is anchored to the reference's own recorded numbers, its float32 instance is measured against its
float64 instance on every shape of the envelope, and the nets it builds have the properties the envelope test relies on.

Measured on the host this was written on (float32 restatement against float64, ten shapes, gains 1 / 4 / 16):
  span-weighted error of hidden planes (vision_reference.span_weighted): root 2.9e-8 .. 6.3e-7 (worst at (2,2,64,6)),
  recurrent 1.7e-7 .. 1.22e-6 (worst at (2,8,36,3): three residual blocks); the towers' gain does not enter either.
  The PLAIN error of the same planes: up to 1.3e-3 at (33,64,63,2) -- 7.8 % of its pixels have a span of exactly 0, 194 a
  span below 1e-3 -- which is why no test of this family holds a scaled plane to a plain atol on fresh nets.
  Pixels on the + 1e-5 discontinuity (left out): at most 0.005 % of a case.
  Largest |policy logit| at gain 16: 1.24 ((2,2,64,6)) .. 9.42 ((1,1,1,0))."""
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import vision_reference as vr
from test_vision_family import TOL, _frame, _net

# 4 x the worst span-weighted float32 error measured where this file was written (module docstring): other hosts sum float32
# convolutions in another order (the project has seen 2.4 x between hosts)
E32W_BOUND = 4 * 1.23e-6


def _rows(fn, *args):
    """fn on every row as a batch of one, as the reference's *_inference functions call the modules: ATen's CPU convolutions sum
    in another order for larger batches, which the scaling of a small-span pixel magnifies beyond 1e-6."""
    outs = [fn(*(torch.as_tensor(a)[i:i + 1] for a in args)) for i in range(len(args[0]))]
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def test_float32_restatement_reproduces_the_reference_tape():
    """The float32 Restatement of visionnet_L1_seed0 against every third network call of vision_sims50.npz, at the tolerances of
    test_vision_family.test_heads_reproduce_the_reference_tape: staging, action plane and branch selection are the
    reference's.  Like that test it compares scaled planes with a plain 1e-6 and so depends on the host's ATen float32
    convolutions summing as on the host that recorded the tape (measured difference: 0 where they do).  On two hosts with
    another summation order both tests miss on a few small-span pixels: this one by 1.61e-6 (2 of 2499 values) and 4.7e-6 on
    hidden planes, 6.6e-7 on root planes and 6.0e-8 on policies; a wrong stage, plane or branch shows at 1e-3 and above."""
    r = vr.Restatement(_net("visionnet_L1_seed0"), torch.float32)
    cfg, cases = gu.cases("vision_sims50")
    sims = np.arange(0, int(cfg["num_simulations"]), 3)
    for c in cases:
        root = r.represent(_frame(3000 + int(c["seed"])))
        np.testing.assert_allclose(root["hidden"].numpy().reshape(-1), c["root_hidden"], atol=TOL, rtol=0)
        pol = r.predict(root["hidden"], torch.ones(1))["policy"]
        np.testing.assert_allclose(pol.numpy()[0], c["root_policy"], atol=TOL, rtol=0)
        h, a, br = c["tape_hidden_in"][sims], c["tape_action"][sims], torch.as_tensor(c["tape_branch"][sims])
        assert br.any() and not br.all()
        out = _rows(r.transition, h, a, br)
        np.testing.assert_allclose(out["hidden"].numpy().reshape(len(sims), -1), c["tape_hidden_out"][sims], atol=TOL, rtol=0)
        np.testing.assert_allclose(out["reward"].numpy(), c["tape_reward"][sims], atol=1e-5, rtol=0)
        assert (out["reward"][br == 0] == 0).all() and (out["reward_logits"][br == 0] == 0).all()
        pre = _rows(r.predict, out["hidden"], br)
        np.testing.assert_allclose(pre["policy"].numpy(), c["tape_policy"][sims], atol=TOL, rtol=0)
        np.testing.assert_allclose(pre["value"].numpy(), c["tape_value"][sims], atol=5e-4, rtol=0)


def test_float32_restatement_reproduces_the_batchnorm_net():
    """visionnet_L2_bn (shared residual block applied twice, three action planes, perturbed batch-norm) against
    visionnet_L2_bn_io.npz at the tolerances of test_vision_family.test_deeper_net_with_batchnorm_statistics."""
    r = vr.Restatement(_net("visionnet_L2_bn"), torch.float32)
    io = np.load(os.path.join(gu.GOLDEN, "visionnet_L2_bn_io.npz"))
    A, n = 3, len(io["obs_seed"])
    root = _rows(r.represent, torch.cat([_frame(s) for s in io["obs_seed"]]))
    np.testing.assert_allclose(root["hidden"].numpy(), io["hidden"], atol=TOL, rtol=0)
    pre = _rows(r.predict, root["hidden"], torch.ones(n))
    np.testing.assert_allclose(pre["policy"].numpy(), io["policy"], atol=TOL, rtol=0)
    np.testing.assert_allclose(pre["value"].numpy(), io["value"].reshape(-1), atol=5e-4, rtol=0)
    h = root["hidden"].repeat_interleave(A, 0)
    a = torch.arange(A).repeat(n)
    aft = _rows(r.transition, h, a, torch.zeros(n * A))
    np.testing.assert_allclose(aft["hidden"].numpy(), io["afterstate"], atol=TOL, rtol=0)
    assert (aft["reward"] == 0).all()
    apre = _rows(r.predict, aft["hidden"], torch.zeros(n * A))
    np.testing.assert_allclose(apre["policy"].numpy(), io["apolicy"], atol=TOL, rtol=0)
    np.testing.assert_allclose(apre["value"].numpy(), io["avalue"].reshape(-1), atol=5e-4, rtol=0)
    dyn = _rows(r.transition, aft["hidden"], a, torch.ones(n * A))
    np.testing.assert_allclose(dyn["reward"].numpy(), io["reward"].reshape(-1), atol=5e-4, rtol=0)
    np.testing.assert_allclose(dyn["hidden"].numpy(), io["next_hidden"], atol=TOL, rtol=0)


@pytest.mark.parametrize("shape", vr.SHAPES, ids=vr.shape_id)
def test_float32_restatement_is_near_the_float64_one_span_weighted(shape):
    """32 frames and 2048 recurrent rows per shape (the hidden planes do not depend on the towers' gain): the span-weighted
    error of the float32 instance -- what the GPU test multiplies by 4 for its bound -- stays below 4 x the worst value
    measured (module docstring), and at most 1 % of the pixels sit on the + 1e-5 discontinuity."""
    c = vr.case(shape, 1)
    for k in ("root_hidden", "hidden"):
        print(f"{vr.shape_id(shape)} {k}: span-weighted float32 error {c['e32w'][k]:.3e}, left out {100 * c['seam'][k]:.4f} %")
        assert c["e32w"][k] <= E32W_BOUND, (k, c["e32w"][k])
        assert c["seam"][k] <= 0.01
    for gain in vr.GAINS[1:]:
        assert vr.case(shape, gain)["e32w"] == c["e32w"]
    f, h, a, br = c["inputs"]
    assert 0.4 <= float(br.float().mean()) <= 0.6 and int(a.max()) == shape[0] - 1


def test_small_spans_of_both_kinds_occur_in_the_cases():
    """Pixels whose three channels are equal after the relu (span exactly 0) and pixels with a span of 1e-5 .. 1e-3: the cases
    the span-weighted rule exists for are part of the inputs the envelope test runs."""
    spans = torch.cat([vr.case(s, 1)[k]["span"].flatten() for s in vr.SHAPES for k in ("root64", "out64")])
    assert int((spans == 0).sum()) > 100 and int(((spans > 1e-5) & (spans < 1e-3)).sum()) > 10


@pytest.mark.parametrize("shape", vr.SHAPES, ids=vr.shape_id)
def test_fresh_net_properties(shape):
    """Perturbed batch-norm statistics in every BatchNorm2d of the five functions, the gain on the last Linear of the five
    towers only, and at gain 16 a largest |policy logit| between 1 and 40: neither a flat nor a saturated softmax."""
    A, S, H, L = shape
    one, big = vr.net_of(shape, 1), vr.net_of(shape, 16)
    norms = vr.batch_norms(one)
    # down-sampler 2, representation 1 + 1 (the branch without down-sampling), transitions 1 each; with hidden layers one
    # residual block more in each transition and each prediction network
    assert len(norms) == (10 if L else 6)
    for bn in norms:
        assert not bn.training
        assert float(bn.running_mean.abs().max()) > 0 and 0.5 <= float(bn.running_var.min()) and float(bn.running_var.max()) <= 1.5
        assert float((bn.weight.detach() - 1).abs().max()) > 0 and float(bn.bias.detach().abs().max()) > 0
    sd1, sd16 = ({k: v for f in vr._FUNCS for k, v in ((f + "." + n, p) for n, p in getattr(m, f + "_function").state_dict().items())}
                 for m in (one, big))
    last = {id(p) for t in vr.towers(big) for p in (t[-1].weight, t[-1].bias)}
    scaled = 0
    for f in vr._FUNCS:
        for (n, p1), (_, p16) in zip(getattr(one, f + "_function").named_parameters(), getattr(big, f + "_function").named_parameters()):
            if id(p16) in last:
                assert torch.equal(p16, p1 * 16), (f, n)
                scaled += 1
            else:
                assert torch.equal(p16, p1), (f, n)
    assert scaled == 10 and set(sd1) == set(sd16)
    c = vr.case(shape, 16)
    f, h, a, br = c["inputs"]
    logits = torch.cat([c["r64"].predict(c["root64"]["hidden"], torch.ones(len(f)))["policy_logits"].flatten(),
                        c["r64"].predict(c["out64"]["hidden"], br)["policy_logits"].flatten()])
    print(f"{vr.shape_id(shape)}: largest |policy logit| at gain 16 = {float(logits.abs().max()):.2f}")
    assert 1 <= float(logits.abs().max()) <= 40
