"""A float64 restatement of the `vision_model` search-side networks, stage by stage, that shares no code with the batched heads.

`Restatement(model)` deep-copies the five compat_vision modules of a Muzero vision_model and casts them to float64 (or, for the
float32 floor of the same arithmetic, leaves them in float32).  The convolutions, batch-norms and towers are the REAL modules
(nn.Conv2d, nn.BatchNorm2d in eval mode, nn.Linear); restated here in the working precision are what surrounds them: the
per-pixel min-max scaling across the channels (span < 1e-5 -> span + 1e-5), the action plane (a + 1) / A, the branch
selection, reward = 0 on afterstate rows, the softmax and the support decode (lstm_reference.decode).

The stages are separate because the scaling divides by the channel span of ONE pixel: after a relu, a few per cent of the
pixels of a fresh net have a span of exactly 0 and a few have spans of 1e-5 .. 1e-3, where a float32 evaluation is 1e-4 away
from the float64 one on the scaled plane although its unscaled planes agree to 1e-7.  So every stage also hands out the span
of its unscaled planes (`span_weighted` undoes the division), and `predict` takes the hidden rows it is to be judged on.

Nothing here goes through heads.HipVisionHeads, its packing or heads.ModuleHeads (helper module, no tests).
"""
import copy
from importlib import import_module

import torch

from lstm_reference import decode

_FUNCS = ("representation", "prediction", "afterstate_prediction", "afterstate_dynamics", "dynamics")
FRAME = (98, 98, 3)
SPAN_FLOOR = 1e-5                    # the weight of a pixel whose span is below the + 1e-5 of the scaling
SPAN_SEAM = (0.5e-5, 2e-5)           # spans on the discontinuity of the scaling: may be left out, at most 1 % of a case


def towers(model):
    """The five Linear towers of the search-side networks (the afterstate dynamics network has no reward branch)."""
    return [model.dynamics_function.sequential_reward[2], model.prediction_function.nn_value[2], model.prediction_function.nn_policy[2],
            model.afterstate_prediction_function.nn_value[2], model.afterstate_prediction_function.nn_policy[2]]


def batch_norms(model):
    """Every BatchNorm2d of the five functions, each shared module once."""
    seen = []
    for f in _FUNCS:
        for m in getattr(model, f + "_function").modules():
            if isinstance(m, torch.nn.BatchNorm2d) and not any(m is s for s in seen):
                seen.append(m)
    return seen


def fresh_net(A, S, H, L, seed=0, gain=1.0):
    """A freshly initialised vision_model in eval mode whose batch-norms are perturbed from a generator seeded with `seed`
    (running mean ~ N(0, 0.2), running variance in [0.5, 1.5], weight ~ 1 + 0.3 N, bias ~ 0.2 N: a fresh net's identity
    batch-norm would hide a swapped scale and shift), and whose five towers have weight and bias of their LAST Linear
    multiplied by `gain`.  (Scaling all L + 2 layers compounds to |logit| ~ 1e4 at gain 16: a saturated softmax tests nothing.)"""
    import stochastic_muzero_amd  # noqa: F401
    model_mod = import_module("stochastic-muzero_amd.model")
    with torch.random.fork_rng():
        torch.manual_seed(int(seed))
        m = model_mod.Muzero(model_structure="vision_model", observation_space_dimensions=FRAME, action_space_dimensions=int(A),
                             state_space_dimensions=int(S), hidden_layer_dimensions=int(H), number_of_hidden_layer=int(L),
                             random_tag=0)
    for f in _FUNCS:
        getattr(m, f + "_function").eval()
    g = torch.Generator().manual_seed(1000 + int(seed))
    with torch.no_grad():
        for bn in batch_norms(m):
            n = bn.num_features
            bn.running_mean.copy_(0.2 * torch.randn(n, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
            bn.weight.copy_(1 + 0.3 * torch.randn(n, generator=g))
            bn.bias.copy_(0.2 * torch.randn(n, generator=g))
        for tower in towers(m):
            tower[-1].weight.mul_(float(gain))
            tower[-1].bias.mul_(float(gain))
    return m


def scale(x):
    """scale_to_bound_action across the channels of [B, C, 7, 7]; also returns the span of every pixel before scaling [B, 7, 7]."""
    lo = x.amin(dim=1, keepdim=True)
    span = x.amax(dim=1, keepdim=True) - lo
    wide = torch.where(span < 1e-5, span + 1e-5, span)
    return (x - lo) / wide, span[:, 0]


def span_weighted(got, want64, span64):
    """(|got - want64| * max(span64, 1e-5) per value of [B, 3, 7, 7] planes (or [B, 147] rows), share of the pixels left
    out because their span sits on the + 1e-5 discontinuity): the statistic on which hidden planes are judged.  The
    left-out pixels weigh 0; pixels of span exactly 0 stay in."""
    B = want64.shape[0]
    got, want64 = torch.as_tensor(got).double().reshape(B, 3, 7, 7), want64.double().reshape(B, 3, 7, 7)
    span64 = span64.double().reshape(B, 1, 7, 7)
    seam = (span64 >= SPAN_SEAM[0]) & (span64 <= SPAN_SEAM[1])
    w = torch.where(seam, torch.zeros_like(span64), span64.clamp(min=SPAN_FLOOR))
    return (got - want64).abs() * w, float(seam.double().mean())


class Restatement:
    def __init__(self, model, dtype=torch.float64):
        self.dtype = dtype
        self.A = int(model.action_dimension)
        mods = [copy.deepcopy(getattr(model, f + "_function")).to("cpu").to(dtype).eval() for f in _FUNCS]
        self.rep, self.pre, self.apr, self.ady, self.dyn = mods

    def _planes(self, hidden):
        h = torch.as_tensor(hidden).to(self.dtype)
        return h.reshape(h.shape[0], 3, 7, 7)

    @torch.no_grad()
    def represent(self, frames):
        """frames [B, 3, 98, 98] -> dict(hidden [B, 3, 7, 7] scaled, span [B, 7, 7] of the unscaled down-sampler output)"""
        hidden, span = scale(self.rep.sequential_downsampler(torch.as_tensor(frames).to(self.dtype)))
        return dict(hidden=hidden, span=span)

    @torch.no_grad()
    def transition(self, hidden, action, branch):
        """hidden [B, 147] or [B, 3, 7, 7], action [B] int, branch [B] (non-zero: dynamics, zero: afterstate dynamics) ->
        dict(hidden scaled, span of the unscaled sequential_container output, reward_logits, reward); reward_logits and
        reward are 0 on afterstate rows."""
        h = self._planes(hidden)
        B = h.shape[0]
        plane = ((torch.as_tensor(action).to(self.dtype) + 1) / self.A).view(B, 1, 1, 1).expand(B, 1, 7, 7)
        x = torch.cat([h, plane], 1)
        m = torch.as_tensor(branch).bool()
        s_dyn, span_dyn = scale(self.dyn.sequential_container(x))
        s_aft, span_aft = scale(self.ady.sequential_container(x))
        rl = self.dyn.sequential_reward(x)
        return dict(hidden=torch.where(m.view(B, 1, 1, 1), s_dyn, s_aft), span=torch.where(m.view(B, 1, 1), span_dyn, span_aft),
                    reward_logits=torch.where(m[:, None], rl, torch.zeros_like(rl)),
                    reward=torch.where(m, decode(rl), torch.zeros(B, dtype=self.dtype)))

    @torch.no_grad()
    def predict(self, hidden, branch):
        """hidden [B, 147] or [B, 3, 7, 7] (scaled), branch [B] (non-zero: prediction, zero: afterstate prediction) ->
        dict(policy, policy_logits, value_logits, value)"""
        h = self._planes(hidden)
        m = torch.as_tensor(branch).bool()
        pp, vp = self.pre(h)
        pa, va = self.apr(h)
        pl, vl = torch.where(m[:, None], pp, pa), torch.where(m[:, None], vp, va)
        return dict(policy=torch.softmax(pl, 1), policy_logits=pl, value_logits=vl, value=decode(vl))


# ---- the cases the envelope tests share (tests/test_vision_reference.py on the CPU, tests/test_gpu_vision_envelope.py) ------
# (A, S, H, L): what each shape is there for is tabulated in tests/test_gpu_vision_envelope.py
SHAPES = ((1, 1, 1, 0), (2, 31, 64, 1), (3, 5, 7, 2), (5, 12, 17, 1), (4, 32, 20, 0), (2, 8, 36, 3), (7, 21, 52, 1),
          (33, 64, 63, 2), (64, 64, 64, 0), (2, 2, 64, 6))
GAINS = (1, 4, 16)
FRAMES, ROWS = 32, 2048
_cache = {}


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def net_of(shape, gain):
    return fresh_net(*shape, seed=400 + SHAPES.index(tuple(shape)), gain=gain)


def inputs_of(shape, rows=ROWS, frames=FRAMES, mode="mixed"):
    """torch.rand frames and hidden rows, random actions, and branches that are mixed (40..60 % dynamics), all dynamics or all
    afterstate dynamics."""
    g = torch.Generator().manual_seed(50 + SHAPES.index(tuple(shape)))
    f = torch.rand(frames, 3, 98, 98, generator=g)
    h = torch.rand(rows, 147, generator=g)
    a = torch.randint(0, shape[0], (rows,), generator=g)
    br = torch.randint(0, 2, (rows,), generator=g)
    assert 0.4 <= float(br.float().mean()) <= 0.6
    if mode != "mixed":
        br = torch.full_like(br, 1 if mode == "dynamics" else 0)
    return f, h, a, br


def case(shape, gain, mode="mixed"):
    """The float64 and float32 restatements of one shape and gain on its inputs, computed once: dict(model, inputs, root64,
    root32, out64, out32, e32w = {"root_hidden", "hidden"}: the span-weighted error of the float32 restatement, seam =
    the share of pixels it left out).  The representation does not depend on the gain (towers only) and is shared."""
    key = (tuple(shape), gain, mode)
    if key not in _cache:
        model = net_of(shape, gain)
        f, h, a, br = inputs_of(shape, mode=mode)
        r64, r32 = Restatement(model), Restatement(model, torch.float32)
        rkey = (tuple(shape), "root")
        if rkey not in _cache:
            _cache[rkey] = (r64.represent(f), r32.represent(f))
        root64, root32 = _cache[rkey]
        out64, out32 = r64.transition(h, a, br), r32.transition(h, a, br)
        e32w, seam = {}, {}
        for name, x64, x32 in (("root_hidden", root64, root32), ("hidden", out64, out32)):
            err, seam[name] = span_weighted(x32["hidden"], x64["hidden"], x64["span"])
            e32w[name] = float(err.max())
        _cache[key] = dict(model=model, inputs=(f, h, a, br), r64=r64, r32=r32, root64=root64, root32=root32, out64=out64,
                           out32=out32, e32w=e32w, seam=seam)
    return _cache[key]


def floor_of(gain):
    """The largest span-weighted float32 error of any shape at this gain, per kind of hidden plane: what keeps a case whose
    float32 restatement happens to be lucky from failing a correct kernel."""
    return {k: max(case(s, gain)["e32w"][k] for s in SHAPES) for k in ("root_hidden", "hidden")}
