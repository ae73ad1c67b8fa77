"""The restatement of tests/mlp_reference.py under the arithmetic of the bf16 broad heads (include/smz.h,
smz_mlp_recurrent_broad_bf16), sharing no code with the packer or the heads (helper module, no tests).

`RoundedRestatement(model, dtype)` is mlp_reference.Restatement -- the REAL compat_mlp modules, deep-copied and cast to `dtype` --
with, in the four recurrent functions,
  * every Linear weight replaced by w.to(torch.bfloat16).to(dtype) (each shared trunk tensor once), and
  * every Linear input passed through x.to(torch.bfloat16).to(dtype) (a forward pre-hook on every nn.Linear: the parent's hidden
    row -- the one-hot part of the input is exact in bf16 -- every ELU output, the scaled state that feeds the prediction network),
biases and everything between the layers in `dtype`; the hidden rows it returns are the unrounded scaled states.  On float32
inputs torch's bf16 cast rounds to nearest even.  dtype float64 is the reference of the bounds, float32 the floor (e32r).  The
representation function is left as it is: the root of these heads is evaluated in float32.
"""
import torch

import mlp_reference as mr


def _to_bf16_and_back(x):
    return x.to(torch.bfloat16).to(x.dtype)


class RoundedRestatement(mr.Restatement):
    def __init__(self, model, dtype=torch.float64):
        super().__init__(model, dtype)
        seen = set()
        for net in (self.pre, self.apr, self.ady, self.dyn):
            for mod in net.modules():
                if isinstance(mod, torch.nn.Linear) and id(mod) not in seen:
                    seen.add(id(mod))
                    with torch.no_grad():
                        mod.weight.copy_(_to_bf16_and_back(mod.weight))
                    mod.register_forward_pre_hook(lambda m, args: (_to_bf16_and_back(args[0]),))
        self.linears = len(seen)
