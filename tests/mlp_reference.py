"""A float64 restatement of the `mlp_model` search-side networks that shares no code with the batched heads.

`Restatement(model)` deep-copies the five function modules of a Muzero mlp_model and casts them to float64 (or, for the
float32 floor of the same arithmetic, leaves them in float32).  Rows are evaluated batched through the REAL modules: the
nn.Sequential trunks of compat_mlp (Linear -> ELU -> the shared Linear(H, H) -> ELU applied number_of_hidden_layer times ->
output Linear).  Around them, restated here in the working precision: scale_to_bound_action (span < 1e-5 -> span + 1e-5; the
span is returned too), softmax, the support decode, the branch selection, and reward = 0 on afterstate rows -- `scale` and
`decode` are those of tests/lstm_reference.py.

Nothing here goes through model.mlp_arrays_from_modules, FusedMlpHeads, the packing of HipMlpHeads / HipMlpTileHeads or the
modules' own forward() (helper module, no tests).
"""
import copy
from importlib import import_module

import torch

from lstm_reference import decode, scale

_FUNCS = ("representation", "prediction", "afterstate_prediction", "afterstate_dynamics", "dynamics")


def fresh_net(obs, A, S, H, L, seed=0, gain=1.0):
    """A freshly initialised mlp_model whose four recurrent functions (every Linear weight and bias) are multiplied by
    `gain`; the representation stays as initialised.  gain 1 = the reference's initial net (N(0, 1/137) weights: outputs
    ~1e-2), larger gains spread the logits like a trained checkpoint's."""
    import stochastic_muzero_amd  # noqa: F401
    model_mod = import_module("stochastic-muzero_amd.model")
    with torch.random.fork_rng():
        torch.manual_seed(int(seed))
        m = model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=int(obs), action_space_dimensions=int(A),
                             state_space_dimensions=int(S), hidden_layer_dimensions=int(H), number_of_hidden_layer=int(L),
                             random_tag=0)
    with torch.no_grad():
        for f in _FUNCS[1:]:
            for p in getattr(m, f + "_function").parameters():      # (parameters(): each shared trunk tensor once)
                p.mul_(float(gain))
    return m


class Restatement:
    def __init__(self, model, dtype=torch.float64):
        self.dtype = dtype
        self.A = int(model.action_dimension)
        mods = [copy.deepcopy(getattr(model, f + "_function")).to("cpu").to(dtype).eval() for f in _FUNCS]
        self.rep, self.pre, self.apr, self.ady, self.dyn = mods

    @torch.no_grad()
    def initial(self, obs):
        """obs [B, obs] -> dict(root_hidden, root_policy, root_span)"""
        x = torch.as_tensor(obs).to(self.dtype)
        hidden, span = scale(self.rep.state_norm(x))
        policy = torch.softmax(self.pre.policy(hidden), 1)
        return dict(root_hidden=hidden, root_policy=policy, root_span=span)

    @torch.no_grad()
    def recurrent(self, hidden_in, action, branch):
        """hidden_in [B, S], action [B] int, branch [B] (non-zero: dynamics + prediction, zero: afterstate pair) ->
        dict(hidden, reward_logits, reward, policy, value_logits, value, span); reward_logits / reward are 0 on afterstate rows."""
        h = torch.as_tensor(hidden_in).to(self.dtype)
        onehot = torch.nn.functional.one_hot(torch.as_tensor(action).long(), self.A).to(self.dtype)
        x = torch.cat([h, onehot], 1)
        m = torch.as_tensor(branch).bool()
        s_dyn, span_dyn = scale(self.dyn.next_state_normalized(x))
        s_aft, span_aft = scale(self.ady.next_state_normalized(x))
        hidden = torch.where(m[:, None], s_dyn, s_aft)
        span = torch.where(m, span_dyn, span_aft)
        rl = self.dyn.reward(x)
        reward_logits = torch.where(m[:, None], rl, torch.zeros_like(rl))
        reward = torch.where(m, decode(rl), torch.zeros_like(span))
        pl = torch.where(m[:, None], self.pre.policy(hidden), self.apr.policy(hidden))
        vl = torch.where(m[:, None], self.pre.value(hidden), self.apr.value(hidden))
        return dict(hidden=hidden, reward_logits=reward_logits, reward=reward, policy=torch.softmax(pl, 1), value_logits=vl,
                    value=decode(vl), span=span)
