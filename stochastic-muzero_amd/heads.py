"""Batched evaluation of the learned heads for all pending leaves of a SearchEngine.

The reference calls five tiny networks once per simulation with batch size 1 (muzero_model.py:802-909).  Here the
same five functions are evaluated once per simulation round for ALL B trees.  Which pair of networks a tree needs
depends on its leaf's parent flag (monte_carlo_tree_search.py:333-342); to keep every shape static (so a whole
search can be captured in one HIP graph) both pairs are evaluated for every tree and the HIP epilogue kernels pick
per tree (smz_dynamics_epilogue / smz_prediction_epilogue).  FLOPs are irrelevant here (~30 kFLOP per leaf).

PyTorch-ROCm is used for the dense layers only; softmax, support decode, min-max scaling and the branch select are
libsmz kernels.

Two implementations of the same interface:
  FusedMlpHeads  -- `mlp_model` family (neural_network_mlp_model.py:5-250): the two dynamics trunks share their
                    input and the two prediction trunks share theirs, so each pair is evaluated as ONE stacked
                    linear layer + ONE block-structured output layer (4 GEMMs per round instead of 10).
  ModuleHeads    -- any head family following the reference's module signatures whose modules treat the rows of a
                    batch independently (vision, ...): calls the five torch modules batched and uses the same
                    epilogues.  Not `lstm_model`: its modules read a 2-D batch as ONE sequence (LstmTorchHeads).
Interface:
  initial(obs)                      -> hidden [B,S] f32, policy [B,A] f32 (softmaxed; the root value is unused, mcts:319)
  recurrent(mlp_input/hidden, last_action, branch) -> hidden' [B,S], reward [B], policy [B,A], value [B]
"""
import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib

# weight names of the mlp_model family as plain arrays: <head>_<layer>_{w,b}
MLP_ARRAYS = ["rep_in", "rep_mid", "rep_out",
              "pre_in", "pre_mid", "pre_pol", "pre_val",
              "apr_in", "apr_mid", "apr_pol", "apr_val",
              "ady_in", "ady_mid", "ady_st",
              "dyn_in", "dyn_mid", "dyn_rw", "dyn_st"]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Heads:
    """What every evaluator shares: the library, the device and the cached output buffers.  A class that a single-launch
    search kernel can take names that kernel's kind in `single_launch` and hands it `single_launch_image()`."""
    single_launch = None        # "mlp", "vision", "lstm", "wide" or "large" (BatchedMCTS.run); None: step-wise searches only

    def __init__(self, device):
        self.lib = _lib.load()
        self.device = torch.device(device)
        self._buf = {}

    def _out(self, name, shape, dtype=torch.float32):
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._buf[name] = torch.empty(*shape, dtype=dtype, device=self.device)
        return t

    def _round_out(self, B, hidden=True):
        """The outputs of one round: hidden' [B,S] (None unless `hidden`), reward [B], policy [B,A], value [B].  The names are
        fixed: a captured graph holds the buffers' addresses."""
        return (self._out("h", (B, self.S)) if hidden else None, self._out("r", (B,)), self._out("p", (B, self.A)),
                self._out("v", (B,)))

    def single_launch_image(self):
        """(descriptor, packed weights) of the single-launch search kernel of this kind."""
        return self.desc, self.weights


def interleave(Wt, width, pad):
    """Wt [K, O <= width] (input-major) -> the flat float32 matrix the kernels read: K padded with zero rows to a multiple of
    `pad` (4 or 8), rows padded with zero columns to `width`, four inputs interleaved -- element (k, o) at
    ((k / 4) * width + o) * 4 + k % 4 (include/smz.h)."""
    import numpy as np
    K, O = Wt.shape
    P = np.zeros(((K + pad - 1) // pad * pad, width), np.float32)
    P[:K, :O] = Wt
    return P.reshape(-1, 4, width).transpose(0, 2, 1).reshape(-1)


# off[] order of smz_mlp_desc: (name of the input-major matrix, [names of the output heads concatenated])
_MATS = [("dyn_in", ["dyn_in"]), ("ady_in", ["ady_in"]), ("dyn_mid", ["dyn_mid"]), ("ady_mid", ["ady_mid"]),
         ("dyn_out", ["dyn_rw", "dyn_st"]), ("ady_out", ["ady_st"]), ("pre_in", ["pre_in"]), ("apr_in", ["apr_in"]),
         ("pre_mid", ["pre_mid"]), ("apr_mid", ["apr_mid"]), ("pre_out", ["pre_pol", "pre_val"]),
         ("apr_out", ["apr_pol", "apr_val"]), ("rep_in", ["rep_in"]), ("rep_mid", ["rep_mid"]), ("rep_out", ["rep_out"])]


def pack_mats(weights, d, pad):
    """The float32 image of smz_mlp_layout (pad 4) / smz_mlp_layout_wide (pad 8) from the torch-layout arrays ([O, K] weights):
    every matrix of _MATS interleaved at d.off[m], its bias at d.off[15 + m]."""
    import numpy as np
    buf = np.zeros(d.total_floats, np.float32)
    for m, (name, parts) in enumerate(_MATS):
        if "_mid" in name and d.L == 0:
            continue
        W = interleave(np.concatenate([np.asarray(weights[p + "_w"], np.float32) for p in parts], 0).T, d.OP, pad)
        b = np.concatenate([np.asarray(weights[p + "_b"], np.float32) for p in parts], 0)
        buf[d.off[m]:d.off[m] + W.size] = W
        buf[d.off[15 + m]:d.off[15 + m] + b.size] = b
    return buf


class FusedMlpHeads(Heads):
    wants_mlp_input, wants_parent_hidden = True, False

    def __init__(self, weights, dims, device):
        """weights: dict name -> array-like ('rep_in_w', 'rep_in_b', ...); dims: obs, A, S, H, L."""
        super().__init__(device)
        self.obs,self.A, self.S, self.H, self.L = (int(dims[k]) for k in ("obs", "A", "S", "H", "L"))
        w = {k: torch.as_tensor(v, dtype=torch.float32).to(self.device) for k, v in weights.items()}
        self.w = w
        A, S, H = self.A, self.S, self.H
        z = lambda r, c: torch.zeros(r, c, device=self.device)
        # representation (mlp:5-42): Linear -> ELU -> [Linear(H,H) -> ELU] x L (one shared module) -> Linear -> scale
        self.rep = [(w["rep_in_w"].t().contiguous(), w["rep_in_b"])] + \
                   [(w["rep_mid_w"].t().contiguous(), w["rep_mid_b"])] * self.L
        self.rep_out = (w["rep_out_w"].t().contiguous(), w["rep_out_b"])
        # root prediction (mlp:47-83): policy and value share the trunk weights
        self.pre = [(w["pre_in_w"].t().contiguous(), w["pre_in_b"])] + \
                   [(w["pre_mid_w"].t().contiguous(), w["pre_mid_b"])] * self.L
        self.pre_pol = (w["pre_pol_w"].t().contiguous(), w["pre_pol_b"])
        # dynamics || afterstate_dynamics, both fed [hidden | one-hot action] (mlp:122-124, 204-206)
        self.dyn_in = (torch.cat([w["dyn_in_w"], w["ady_in_w"]], 0).t().contiguous(),
                       torch.cat([w["dyn_in_b"], w["ady_in_b"]]))
        self.dyn_mid = (torch.block_diag(w["dyn_mid_w"], w["ady_mid_w"]).t().contiguous(),
                        torch.cat([w["dyn_mid_b"], w["ady_mid_b"]]))
        w2 = torch.cat([torch.cat([w["dyn_rw_w"], z(S, H)], 1),     # reward logits      <- dynamics trunk
                        torch.cat([w["dyn_st_w"], z(S, H)], 1),     # next state         <- dynamics trunk
                        torch.cat([z(S, H), w["ady_st_w"]], 1)], 0)  # afterstate         <- afterstate trunk
        self.dyn_out = (w2.t().contiguous(), torch.cat([w["dyn_rw_b"], w["dyn_st_b"], w["ady_st_b"]]))
        # prediction || afterstate_prediction on the chosen next state
        self.prd_in = (torch.cat([w["pre_in_w"], w["apr_in_w"]], 0).t().contiguous(),
                       torch.cat([w["pre_in_b"], w["apr_in_b"]]))
        self.prd_mid = (torch.block_diag(w["pre_mid_w"], w["apr_mid_w"]).t().contiguous(),
                        torch.cat([w["pre_mid_b"], w["apr_mid_b"]]))
        w3 = torch.cat([torch.cat([w["pre_pol_w"], z(A, H)], 1), torch.cat([w["pre_val_w"], z(S, H)], 1),
                        torch.cat([z(A, H), w["apr_pol_w"]], 1), torch.cat([z(S, H), w["apr_val_w"]], 1)], 0)
        self.prd_out = (w3.t().contiguous(),
                        torch.cat([w["pre_pol_b"], w["pre_val_b"], w["apr_pol_b"], w["apr_val_b"]]))

    @classmethod
    def from_npz(cls, path, device):
        import numpy as np
        z = np.load(path)
        dims = {k: int(z["dim_" + k]) for k in ("obs", "A", "S", "H", "L")}
        weights = {n + s: z[n + s] for n in MLP_ARRAYS for s in ("_w", "_b")}
        return cls(weights, dims, device)

    @staticmethod
    def _trunk(x, layers):
        for wt, b in layers:
            x = F.elu(torch.addmm(b, x, wt))
        return x

    def initial(self, obs):
        B = obs.shape[0]
        pre = torch.addmm(self.rep_out[1], self._trunk(obs, self.rep), self.rep_out[0])     # [B,S] pre-scale
        hidden = self._out("h0", (B, self.S))
        zero = self._out("zero_branch", (B,), torch.uint8)
        zero.zero_()
        # scale_to_bound_action through the same epilogue (afterstate slot, branch 0, no reward)
        _lib.check(self.lib.smz_dynamics_epilogue(_ptr(pre), _ptr(pre), None, self.S, _ptr(zero), self.S, _ptr(hidden),
                                                  None, B, _stream(self.device)))
        logits = torch.addmm(self.pre_pol[1], self._trunk(hidden, self.pre), self.pre_pol[0])
        policy = self._out("p0", (B, self.A))
        _lib.check(self.lib.smz_policy_softmax(_ptr(logits), self.A, _ptr(policy), B, _stream(self.device)))
        return hidden, policy

    def recurrent(self, engine):
        """Consumes engine.mlp_input / engine.branch (outputs of the last select); returns the four tensors that
        smz_expand_backup takes."""
        x, branch = engine.mlp_input, engine.branch
        B, A, S = x.shape[0], self.A, self.S
        hidden, reward, policy, value = self._round_out(B)
        t = F.elu(torch.addmm(self.dyn_in[1], x, self.dyn_in[0]))
        for _ in range(self.L):
            t = F.elu(torch.addmm(self.dyn_mid[1], t, self.dyn_mid[0]))
        o = torch.addmm(self.dyn_out[1], t, self.dyn_out[0])                                 # [B, 3S]
        fs = o.element_size()
        base = o.data_ptr()
        _lib.check(self.lib.smz_dynamics_epilogue(C.c_void_p(base + S * fs), C.c_void_p(base + 2 * S * fs),
                                                  C.c_void_p(base), 3 * S, _ptr(branch), S, _ptr(hidden), _ptr(reward),
                                                  B, _stream(self.device)))
        u = F.elu(torch.addmm(self.prd_in[1], hidden, self.prd_in[0]))
        for _ in range(self.L):
            u = F.elu(torch.addmm(self.prd_mid[1], u, self.prd_mid[0]))
        q = torch.addmm(self.prd_out[1], u, self.prd_out[0])                                 # [B, 2A+2S]
        qb = q.data_ptr()
        _lib.check(self.lib.smz_prediction_epilogue(C.c_void_p(qb), C.c_void_p(qb + A * fs), C.c_void_p(qb + (A + S) * fs),
                                                    C.c_void_p(qb + (2 * A + S) * fs), 2 * A + 2 * S, _ptr(branch), A, S,
                                                    _ptr(policy), _ptr(value), B, _stream(self.device)))
        return hidden, reward, policy, value


class HipMlpHeads(Heads):
    """`mlp_model` heads evaluated by ONE hand-written HIP kernel per phase (smz_mlp_initial / smz_mlp_recurrent):
    weights packed once into the LDS layout described in include/smz.h, no library GEMMs, no torch ops.
    Raises ValueError when the networks do not fit a CU's LDS (use FusedMlpHeads then)."""
    wants_mlp_input, wants_parent_hidden = True, False
    single_launch = "mlp"
    IN_PLACE_MIN = 8192       # from this many trees on (shipped network shape) the rows stay in the tree: see bind_engine
    _MATS = _MATS

    def __init__(self, weights, dims, device):
        super().__init__(device)
        self.obs, self.A, self.S, self.H, self.L = (int(dims[k]) for k in ("obs", "A", "S", "H", "L"))
        d = _lib.MlpDesc(self.obs, self.A, self.S, self.H, self.L)
        if self.lib.smz_mlp_layout(C.byref(d)) != 0:
            raise ValueError("mlp heads do not fit the LDS-resident kernel (use FusedMlpHeads)")
        self.desc = d
        self.weights = torch.from_numpy(pack_mats(weights, d, 4)).to(self.device)
        self._in_place = None

    def initial(self, obs):
        B = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.obs
        hidden, policy = self._out("h0", (B, self.S)), self._out("p0", (B, self.A))
        _lib.check(self.lib.smz_mlp_initial(C.byref(self.desc), _ptr(self.weights), _ptr(obs), _ptr(hidden), _ptr(policy),
                                            B, _stream(self.device)))
        return hidden, policy

    def bind_engine(self, engine):
        """Called by the step-wise search before its first selection.  Large batches of the shipped network shape
        (S 31, H 64, L 0; 2 or 4 actions): the matrix-core kernel reads each leaf's parent row from the tree's
        hidden-state storage and writes the new row into it (smz_mlp_recurrent_rows), so the tree kernels gather and
        scatter no rows -- a quarter of their memory traffic at 10^6 trees.  Returns the row arguments of the tree calls."""
        import os
        lim = int(os.environ.get("SMZ_MLP_IN_PLACE_MIN", self.IN_PLACE_MIN))
        shape_ok = self.S == 31 and self.H == 64 and self.L == 0 and self.A in (2, 4)
        in_place = shape_ok and lim >= 0 and engine.B >= lim and hasattr(self.lib, "smz_mlp_recurrent_rows")
        engine.enable_leaf_ids(in_place)
        self._in_place = engine if in_place else None
        return dict(want_mlp_input=not in_place, want_parent_hidden=False)

    def recurrent(self, engine):
        in_place = self._in_place is engine
        B = engine.B if in_place else engine.mlp_input.shape[0]
        hidden, reward, policy, value = self._round_out(B, hidden=not in_place)     # (in place: the rows stay in the tree)
        if in_place:
            base, n, hs = engine.hidden_layout()
            _lib.check(self.lib.smz_mlp_recurrent_rows(C.byref(self.desc), _ptr(self.weights), base, n, hs, _ptr(engine.leaf_ids),
                                                       _ptr(engine.last_action), _ptr(engine.branch), _ptr(reward), _ptr(policy),
                                                       _ptr(value), B, _stream(self.device)))
            return None, reward, policy, value
        x, branch = engine.mlp_input, engine.branch
        _lib.check(self.lib.smz_mlp_recurrent(C.byref(self.desc), _ptr(self.weights), _ptr(x), _ptr(branch), _ptr(hidden),
                                              _ptr(reward), _ptr(policy), _ptr(value), B, _stream(self.device)))
        return hidden, reward, policy, value


HIP_ROOT_MAX_OBS = 1024     # smz_mlp_initial_wide / _large / _broad: the observation tile lives in LDS


class HipRootLimit(ValueError):
    """hip_root=True asked for an observation wider than HIP_ROOT_MAX_OBS: an explicit opt-in never falls back."""


def _check_hip_root(lib, obs, entry):
    if not hasattr(lib, entry):
        raise RuntimeError(f"libsmz.so does not export {entry} (hip_root=True needs it)")
    if obs > HIP_ROOT_MAX_OBS:
        raise HipRootLimit(f"hip_root=True: observations of {obs} floats exceed the limit of {HIP_ROOT_MAX_OBS} of {entry}")


def _hip_initial(heads, entry, desc, obs, packed=None):
    """FusedMlpHeads.initial as ONE launch of `entry` on the packed image (heads.packed unless the root has an image of its
    own), into the same cached h0 / p0 buffers."""
    B = obs.shape[0]
    assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == heads.obs
    hidden, policy = heads._out("h0", (B, heads.S)), heads._out("p0", (B, heads.A))
    _lib.check(getattr(heads.lib, entry)(C.byref(desc), _ptr(heads.packed if packed is None else packed), _ptr(obs), _ptr(hidden),
                                         _ptr(policy), B, _stream(heads.device)))
    return hidden, policy


class HipMlpTileHeads(FusedMlpHeads):
    """`mlp_model` heads too wide for the LDS-resident kernels (H <= 128, 2 S <= 128, any number_of_hidden_layer: the
    reference's config 434, S 61 / H 126 / L 0, and its checkpoint 450, L 4): the recurrent networks as ONE hand-written kernel per simulation round
    (smz_mlp_recurrent_wide: 16-leaf tiles on the matrix cores, weights streamed from L2 in the 128-wide packed layout of
    smz_mlp_layout_wide) instead of ten library launches; the root evaluation stays on the torch GEMMs of FusedMlpHeads
    (once per search) unless hip_root=True (opt-in): then it is ONE launch on the same packed image (smz_mlp_initial_wide;
    observations of up to 1024 floats, ValueError above), equal to the torch root within float32 rounding, not bit for bit.
    Raises ValueError outside the kernel's limits."""
    wants_mlp_input, wants_parent_hidden = True, False
    single_launch = "wide"

    def __init__(self, weights, dims, device, hip_root=False):
        super().__init__(weights, dims, device)
        self.hip_root = bool(hip_root)
        d = _lib.MlpDesc(int(dims["obs"]), self.A, self.S, self.H, self.L)
        if not hasattr(self.lib, "smz_mlp_layout_wide") or self.lib.smz_mlp_layout_wide(C.byref(d)) != 0:
            raise ValueError("mlp heads outside the limits of the wide tile kernel (use FusedMlpHeads)")
        self.wide_desc = d
        if self.hip_root:
            _check_hip_root(self.lib, self.obs, "smz_mlp_initial_wide")
            # (bound on the instance: without the flag `initial` stays FusedMlpHeads.initial itself)
            self.initial = lambda obs: _hip_initial(self, "smz_mlp_initial_wide", self.wide_desc, obs)
        self.packed = torch.from_numpy(pack_mats(weights, d, 8)).to(self.device)

    def single_launch_image(self):
        return self.wide_desc, self.packed

    def recurrent(self, engine):
        x, branch = engine.mlp_input, engine.branch
        B = x.shape[0]
        hidden, reward, policy, value = self._round_out(B)
        _lib.check(self.lib.smz_mlp_recurrent_wide(C.byref(self.wide_desc), _ptr(self.packed), _ptr(x), _ptr(branch), _ptr(hidden),
                                                   _ptr(reward), _ptr(policy), _ptr(value), B, _stream(self.device)))
        return hidden, reward, policy, value


class HipMlpLargeHeads(FusedMlpHeads):
    """`mlp_model` heads for up to 1024 actions (H <= 128, 2 S <= 128, no limit on A + S): the recurrent networks as ONE
    hand-written kernel per simulation round (smz_mlp_recurrent_large, csrc/smz_mlp_large.hip) on the parent's hidden row and
    the action itself -- select writes no [B, S + A] one-hot input.  The packed image is that of smz_mlp_layout_large
    (include/smz.h): the two input matrices as a hidden part + an action table, the two prediction output matrices as
    128-column panels.  The root evaluation stays on the torch GEMMs of FusedMlpHeads (once per search) unless
    hip_root=True (opt-in): then it is ONE launch on the same packed image (smz_mlp_initial_large; observations of up to 1024
    floats, ValueError above).  Opt-in (Muzero.heads(backend="large")).  Raises ValueError outside the kernel's limits."""
    wants_mlp_input, wants_parent_hidden = False, True
    single_launch = "large"

    def __init__(self, weights, dims, device, hip_root=False):
        super().__init__(weights, dims, device)
        self.hip_root = bool(hip_root)
        d = _lib.MlpDesc(int(dims["obs"]), self.A, self.S, self.H, self.L)
        if not hasattr(self.lib, "smz_mlp_layout_large") or self.lib.smz_mlp_layout_large(C.byref(d)) != 0:
            raise ValueError("mlp heads outside the limits of the large-action tile kernel (A <= 1024, H <= 128, 2 S <= 128)")
        self.large_desc = d
        if self.hip_root:
            _check_hip_root(self.lib, self.obs, "smz_mlp_initial_large")
            # (bound on the instance: without the flag `initial` stays FusedMlpHeads.initial itself)
            self.initial = lambda obs: _hip_initial(self, "smz_mlp_initial_large", self.large_desc, obs)
        self.packed = torch.from_numpy(self.pack(weights, d)).to(self.device)

    def single_launch_image(self):
        return self.large_desc, self.packed

    @staticmethod
    def pack(weights, d):
        """The float32 image smz_mlp_layout_large describes, from the torch-layout arrays ([O, K] weights)."""
        import numpy as np
        A, S, OP = d.A, d.S, d.OP
        r8 = lambda k: (k + 7) & ~7
        buf = np.zeros(d.total_floats, np.float32)

        def wide(at, Wt):
            """Wt [K, O <= OP] input-major -> the interleaved wide matrix at float offset `at`, K padded to 8."""
            img = interleave(Wt, OP, 8)
            buf[at:at + img.size] = img

        for m, (name, parts) in enumerate(_MATS):
            if "_mid" in name and d.L == 0:
                continue
            W = [np.asarray(weights[p + "_w"], np.float32) for p in parts]          # [O, K] each
            b = [np.asarray(weights[p + "_b"], np.float32) for p in parts]
            at, bias = d.off[m], d.off[15 + m]
            if name in ("dyn_in", "ady_in"):            # hidden part, then the action table [A][OP]
                Wt = W[0].T                             # [S + A, H]
                wide(at, Wt[:S])
                table = np.zeros((A, OP), np.float32)
                table[:, :Wt.shape[1]] = Wt[S:]
                buf[at + r8(S) * OP:at + (r8(S) + A) * OP] = table.reshape(-1)
                buf[bias:bias + b[0].size] = b[0]
            elif name in ("pre_out", "apr_out"):        # policy panels of OP columns, then the value panel
                H = W[0].shape[1]
                panels = (A + OP - 1) // OP
                for p in range(panels):
                    lo, hi = p * OP, min(A, (p + 1) * OP)
                    wide(at + p * r8(H) * OP, W[0][lo:hi].T)
                    buf[bias + p * OP:bias + p * OP + hi - lo] = b[0][lo:hi]
                wide(at + panels * r8(H) * OP, W[1].T)
                buf[bias + panels * OP:bias + panels * OP + S] = b[1]
            else:
                wide(at, np.concatenate(W, 0).T)
                bb = np.concatenate(b, 0)
                buf[bias:bias + bb.size] = bb
        return buf

    def recurrent(self, engine):
        ph, branch = engine.parent_hidden, engine.branch
        B = ph.shape[0]
        assert ph.dtype == torch.float32 and ph.is_contiguous() and ph.shape[1] == self.S
        hidden, reward, policy, value = self._round_out(B)
        _lib.check(self.lib.smz_mlp_recurrent_large(C.byref(self.large_desc), _ptr(self.packed), _ptr(ph), _ptr(engine.last_action),
                                                    _ptr(branch), _ptr(hidden), _ptr(reward), _ptr(policy), _ptr(value), B,
                                                    _stream(self.device)))
        return hidden, reward, policy, value


class HipMlpBroadHeads(FusedMlpHeads):
    """`mlp_model` heads up to 512 wide (hidden_layer_dimensions <= 512, state_space_dimensions <= 256, up to 1024 actions):
    the recurrent networks as ONE hand-written kernel per simulation round (smz_mlp_recurrent_broad, csrc/smz_mlp_broad.hip)
    on the parent's hidden row and the action itself.  Every layer of the packed image (smz_mlp_layout_broad, include/smz.h)
    is a sequence of 128-column panels; the input matrices are a hidden part + an action table.  The root evaluation is
    FusedMlpHeads.initial, on the torch GEMMs (once per search), unless hip_root=True (opt-in): then it is ONE launch on the
    same packed image (smz_mlp_initial_broad, csrc/smz_mlp_broad_root.hip; observations of up to 1024 floats, ValueError
    above), equal to the torch root within float32 rounding, not bit for bit.  No single-launch search takes these heads.
    Opt-in (Muzero.heads(backend="broad")).  Raises ValueError outside the kernel's limits."""
    wants_mlp_input, wants_parent_hidden = False, True
    single_launch = None

    def __init__(self, weights, dims, device, hip_root=False):
        super().__init__(weights, dims, device)
        self.hip_root = bool(hip_root)
        d = _lib.MlpDesc(int(dims["obs"]), self.A, self.S, self.H, self.L)
        if not hasattr(self.lib, "smz_mlp_layout_broad") or self.lib.smz_mlp_layout_broad(C.byref(d)) != 0:
            raise ValueError("mlp heads outside the limits of the broad tile kernel (H <= 512, S <= 256, A <= 1024)")
        self.broad_desc = d
        if self.hip_root:
            _check_hip_root(self.lib, self.obs, "smz_mlp_initial_broad")
            # (bound on the instance: without the flag `initial` stays FusedMlpHeads.initial itself)
            self.initial = lambda obs: _hip_initial(self, "smz_mlp_initial_broad", self.broad_desc, obs)
        self.packed = torch.from_numpy(self.pack(weights, d)).to(self.device)

    @staticmethod
    def pack(weights, d):
        """The float32 image smz_mlp_layout_broad describes, from the torch-layout arrays ([O, K] weights)."""
        import numpy as np
        A, S, H, OP = d.A, d.S, d.H, d.OP
        r8 = lambda k: (k + 7) & ~7
        P = lambda n: (n + OP - 1) // OP
        buf = np.zeros(d.total_floats, np.float32)

        def panels(at, bias, W, b):
            """W [O, K], b [O] -> P(O) panels of r8(K) x OP floats at `at`, one bias vector of OP floats per panel at `bias`;
            returns the float offsets behind them."""
            O, K = W.shape
            for p in range(P(O)):
                lo, hi = p * OP, min(O, (p + 1) * OP)
                img = interleave(W[lo:hi].T, OP, 8)
                buf[at:at + img.size] = img
                buf[bias:bias + hi - lo] = b[lo:hi]
                at, bias = at + r8(K) * OP, bias + OP
            return at, bias

        for m, (name, parts) in enumerate(_MATS):
            if "_mid" in name and d.L == 0:
                continue
            W = [np.asarray(weights[p + "_w"], np.float32) for p in parts]          # [O, K] each
            b = [np.asarray(weights[p + "_b"], np.float32) for p in parts]
            at, bias = d.off[m], d.off[15 + m]
            if name in ("dyn_in", "ady_in"):            # hidden part, then the action table [A][OP * P(H)]
                at, _ = panels(at, bias, W[0][:, :S], b[0])
                table = np.zeros((A, OP * P(H)), np.float32)
                table[:, :H] = W[0][:, S:].T
                buf[at:at + table.size] = table.reshape(-1)
            else:                                       # each part in panels of its own: reward | state, policy | value
                for Wp, bp in zip(W, b):
                    at, bias = panels(at, bias, Wp, bp)
        return buf

    def recurrent(self, engine):
        ph, branch = engine.parent_hidden, engine.branch
        B = ph.shape[0]
        assert ph.dtype == torch.float32 and ph.is_contiguous() and ph.shape[1] == self.S
        hidden, reward, policy, value = self._round_out(B)
        _lib.check(self.lib.smz_mlp_recurrent_broad(C.byref(self.broad_desc), _ptr(self.packed), _ptr(ph), _ptr(engine.last_action),
                                                    _ptr(branch), _ptr(hidden), _ptr(reward), _ptr(policy), _ptr(value), B,
                                                    _stream(self.device)))
        return hidden, reward, policy, value


class HipMlpBroadBf16Heads(FusedMlpHeads):
    """HipMlpBroadHeads' envelope (hidden_layer_dimensions <= 512, state_space_dimensions <= 256, up to 1024 actions) with bf16
    operands on the matrix cores: ONE launch of smz_mlp_recurrent_broad_bf16 (csrc/smz_mlp_broad_bf16.hip) per simulation round.
    The arithmetic is the contract of include/smz.h, not torch.autocast's: weights rounded to bf16 (nearest even) once, here in
    pack(); every Linear input rounded to bf16 in the kernel; biases, accumulation, ELU, scaling, softmax and support decodes in
    float32; the hidden rows handed back to the tree are unrounded float32.  The root evaluation is FusedMlpHeads.initial, in
    float32 on the torch GEMMs (once per search), unless hip_root=True (opt-in): then it is ONE launch of
    smz_mlp_initial_broad, still in float32 -- the bf16 contract covers the recurrent networks alone -- on a float32 image
    of its own, HipMlpBroadHeads.pack on a smz_mlp_layout_broad descriptor (root_desc / root_packed, built only with the
    flag): the root is bit for bit that of HipMlpBroadHeads.  Extra device memory with the flag: the whole float32 image,
    a few MB for most shapes, 15 MB at the envelope's corner (obs 1024, A 1024, S 256, H 512; 20 MB with L > 0).  Observations
    of up to 1024 floats, ValueError above.  No single-launch search takes these heads.  Opt-in
    (Muzero.heads(backend="broad_bf16")).  Raises ValueError outside the kernel's limits."""
    wants_mlp_input, wants_parent_hidden = False, True
    single_launch = None

    def __init__(self, weights, dims, device, hip_root=False):
        super().__init__(weights, dims, device)
        self.hip_root = bool(hip_root)
        d = _lib.MlpDesc(int(dims["obs"]), self.A, self.S, self.H, self.L)
        if not hasattr(self.lib, "smz_mlp_layout_broad_bf16") or self.lib.smz_mlp_layout_broad_bf16(C.byref(d)) != 0:
            raise ValueError("mlp heads outside the limits of the bf16 broad tile kernel (H <= 512, S <= 256, A <= 1024)")
        self.broad_bf16_desc = d
        if self.hip_root:
            _check_hip_root(self.lib, self.obs, "smz_mlp_initial_broad")
            r = _lib.MlpDesc(int(dims["obs"]), self.A, self.S, self.H, self.L)
            if self.lib.smz_mlp_layout_broad(C.byref(r)) != 0:
                raise ValueError("mlp heads outside the limits of the broad tile kernel (H <= 512, S <= 256, A <= 1024)")
            self.root_desc = r
            self.root_packed = torch.from_numpy(HipMlpBroadHeads.pack(weights, r)).to(self.device)
            # (bound on the instance: without the flag `initial` stays FusedMlpHeads.initial itself)
            self.initial = lambda obs: _hip_initial(self, "smz_mlp_initial_broad", self.root_desc, obs, self.root_packed)
        self.packed = torch.from_numpy(self.pack(weights, d).view("int32")).to(self.device)

    @staticmethod
    def round_bf16(x):
        """float32 array -> uint16 array of bf16 bit patterns, round-to-nearest-even (NaN stays NaN)."""
        import numpy as np
        u = np.ascontiguousarray(x, np.float32).view(np.uint32)
        r = ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
        nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
        return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)

    @staticmethod
    def pack(weights, d):
        """The image smz_mlp_layout_broad_bf16 describes as uint32 words, from the torch-layout arrays ([O, K] weights): float32
        bit patterns for the biases, pairs of bf16 (low half first) everywhere else."""
        import numpy as np
        A, S, H, OP = d.A, d.S, d.H, d.OP
        r32 = lambda k: (k + 31) & ~31
        P = lambda n: (n + OP - 1) // OP
        words = np.zeros(d.total_floats, np.uint32)
        halves, floats = words.view(np.uint16), words.view(np.float32)      # (little endian: element e of word w at 2 w + e)

        def panels(at, bias, W, b):
            """W [O, K], b [O] -> P(O) panels of r32(K) x OP bf16 at word `at`, one bias vector of OP floats per panel at word
            `bias`; returns the word offsets behind them."""
            O, K = W.shape
            for p in range(P(O)):
                lo, hi = p * OP, min(O, (p + 1) * OP)
                full = np.zeros((r32(K), OP), np.float32)                   # [k][o]
                full[:K, :hi - lo] = W[lo:hi].T
                # [step][k % 32 / 8][k % 8][tile][o % 16] -> [step][tile][k % 32 / 8][o % 16][k % 8]
                img = full.reshape(r32(K) // 32, 4, 8, OP // 16, 16).transpose(0, 3, 1, 4, 2)
                halves[2 * at:2 * at + img.size] = HipMlpBroadBf16Heads.round_bf16(img.reshape(-1))
                floats[bias:bias + hi - lo] = b[lo:hi]
                at, bias = at + r32(K) * OP // 2, bias + OP
            return at, bias

        for m, (name, parts) in enumerate(_MATS):
            if "_mid" in name and d.L == 0:
                continue
            W = [np.asarray(weights[p + "_w"], np.float32) for p in parts]          # [O, K] each
            b = [np.asarray(weights[p + "_b"], np.float32) for p in parts]
            at, bias = d.off[m], d.off[15 + m]
            if name in ("dyn_in", "ady_in"):            # hidden part, then the action table [A][OP * P(H)] bf16
                at, _ = panels(at, bias, W[0][:, :S], b[0])
                table = np.zeros((A, OP * P(H)), np.float32)
                table[:, :H] = W[0][:, S:].T
                halves[2 * at:2 * at + table.size] = HipMlpBroadBf16Heads.round_bf16(table.reshape(-1))
            else:                                       # each part in panels of its own: reward | state, policy | value
                for Wp, bp in zip(W, b):
                    at, bias = panels(at, bias, Wp, bp)
        return words

    def recurrent(self, engine):
        ph, branch = engine.parent_hidden, engine.branch
        B = ph.shape[0]
        assert ph.dtype == torch.float32 and ph.is_contiguous() and ph.shape[1] == self.S
        hidden, reward, policy, value = self._round_out(B)
        _lib.check(self.lib.smz_mlp_recurrent_broad_bf16(C.byref(self.broad_bf16_desc), _ptr(self.packed), _ptr(ph),
                                                         _ptr(engine.last_action), _ptr(branch), _ptr(hidden), _ptr(reward),
                                                         _ptr(policy), _ptr(value), B, _stream(self.device)))
        return hidden, reward, policy, value


class HipVisionHeads(Heads):
    """`vision_model` heads (the reference's ResNet-v2 family, compat_vision.py) evaluated by hand-written HIP kernels:
    smz_vision_initial (one workgroup per frame) and smz_vision_recurrent (one wavefront per leaf).  Weights are
    packed once from the five modules into the layout documented at smz_vision_desc (include/smz.h)."""
    wants_mlp_input, wants_parent_hidden = False, True
    single_launch = "vision"
    is_rgb = True
    records_frames = True       # initial(obs, record=...) appends the frames to the trajectory record in the same launch
    # index constants of include/smz.h
    _T = dict(CONV_IN=0, BN_IN=1, RES_A=2, RES_B=3, RES_BN=4, MIX_W=5, MIX_B=6, TOWER=7, STRIDE=13, BASE=0)
    _P = dict(RES_A=0, RES_B=1, RES_BN=2, VMIX_W=3, VMIX_B=4, VTOWER=5, PMIX_W=11, PMIX_B=12, PTOWER=13, STRIDE=19, BASE=26)
    _R = dict(STEM=0, NARROW_A=1, NARROW_B=2, NARROW_BN=3, WIDEN=4, WIDE_A=5, WIDE_B=6, WIDE_BN=7, LAST_A=8, LAST_B=9,
              LAST_BN=10, BASE=64)

    def __init__(self, representation, prediction, afterstate_prediction, afterstate_dynamics, dynamics, num_actions,
                 support_size, device):
        import numpy as np
        super().__init__(device)
        tower = dynamics.sequential_reward[2]
        linears = [m for m in tower if isinstance(m, torch.nn.Linear)]
        self.A, self.Ssup, self.H = int(num_actions), int(support_size), int(linears[0].out_features)
        self.L = (len(tower) - 3) // 2                  # [Linear, relu] + [Linear, relu] * L + [Linear]
        if linears[0].in_features != 147 or not getattr(representation, "down_sampling", True):
            raise ValueError("the HIP vision kernels cover the down-sampling family (98x98x3 frames, 3x7x7 hidden state)")
        d = _lib.VisionDesc(self.A, self.Ssup, self.H, self.L)
        if self.lib.smz_vision_layout(C.byref(d)) != 0:
            raise ValueError("vision heads outside the kernel's limits (A, S, H <= 64)")
        self.desc, self.S = d, 147
        buf = np.zeros(d.total_floats, np.float32)
        OP = d.OP

        def put(idx, arr):
            a = np.asarray(arr.detach().cpu().numpy() if torch.is_tensor(arr) else arr, np.float32).reshape(-1)
            buf[d.off[idx]:d.off[idx] + a.size] = a

        def put_bn(idx, bn):
            # ATen's CPU eval-mode batch-norm: alpha = weight * (1 / sqrt(var + eps)), beta = bias - mean * alpha (float32)
            var, mean = bn.running_var.detach().cpu().numpy().astype(np.float32), bn.running_mean.detach().cpu().numpy().astype(np.float32)
            invstd = (np.float32(1) / np.sqrt(var + np.float32(bn.eps))).astype(np.float32)
            w = bn.weight.detach().cpu().numpy().astype(np.float32) if bn.affine else np.ones_like(var)
            b = bn.bias.detach().cpu().numpy().astype(np.float32) if bn.affine else np.zeros_like(var)
            alpha = (w * invstd).astype(np.float32)
            put(idx, np.concatenate([alpha, (b - mean * alpha).astype(np.float32)]))

        def put_linear(idx, lin):
            put(idx, interleave(lin.weight.detach().cpu().numpy().astype(np.float32).T, OP, 4))
            put(idx + 1, lin.bias)

        def put_tower(idx, seq):
            lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
            put_linear(idx, lins[0])
            if self.L > 0:
                put_linear(idx + 2, lins[1])
            put_linear(idx + 4, lins[-1])

        def put_block(ia, ib, ibn, block):
            sc = block.sequential_container         # bn, relu, convA, bn, relu, convB, bn, relu, convA
            put(ia, sc[2].weight); put(ib, sc[5].weight); put_bn(ibn, sc[0])

        T, P, R = self._T, self._P, self._R
        for n, mod in enumerate((dynamics, afterstate_dynamics)):
            b = T["BASE"] + n * T["STRIDE"]
            sc = mod.sequential_container           # conv, bn, relu, [block] * L, relu
            put(b + T["CONV_IN"], sc[0].weight); put_bn(b + T["BN_IN"], sc[1])
            if self.L > 0:
                put_block(b + T["RES_A"], b + T["RES_B"], b + T["RES_BN"], sc[3])
            if n == 0:
                rw = mod.sequential_reward          # conv1x1, flatten, tower
                put(b + T["MIX_W"], rw[0].weight); put(b + T["MIX_B"], rw[0].bias); put_tower(b + T["TOWER"], rw[2])
        for n, mod in enumerate((prediction, afterstate_prediction)):
            b = P["BASE"] + n * P["STRIDE"]
            if self.L > 0:
                put_block(b + P["RES_A"], b + P["RES_B"], b + P["RES_BN"], mod.resnet[0])
            put(b + P["VMIX_W"], mod.nn_value[0].weight); put(b + P["VMIX_B"], mod.nn_value[0].bias)
            put_tower(b + P["VTOWER"], mod.nn_value[2])
            put(b + P["PMIX_W"], mod.nn_policy[0].weight); put(b + P["PMIX_B"], mod.nn_policy[0].bias)
            put_tower(b + P["PTOWER"], mod.nn_policy[2])
        down = representation.sequential_downsampler[0].sequential_container   # stem, R1, R1, widen, R2, R2, pool, R2 x3, pool
        b = R["BASE"]
        put(b + R["STEM"], down[0].weight); put_block(b + R["NARROW_A"], b + R["NARROW_B"], b + R["NARROW_BN"], down[1])
        put(b + R["WIDEN"], down[3].weight); put_block(b + R["WIDE_A"], b + R["WIDE_B"], b + R["WIDE_BN"], down[4])
        put_block(b + R["LAST_A"], b + R["LAST_B"], b + R["LAST_BN"], representation.sequential_downsampler[1])
        self.weights = torch.from_numpy(buf).to(self.device)

    def initial(self, obs, record=None):
        """`record` ([B, 3*98*98] or [B,3,98,98] float32, contiguous): the launch also copies the frames there -- the trajectory
        record of the observation, written by the threads that read it (smz_vision_initial_record)."""
        B = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.is_contiguous() and tuple(obs.shape[1:]) == (3, 98, 98)
        assert record is None or (record.dtype == torch.float32 and record.is_contiguous() and record.numel() == obs.numel())
        hidden, policy = self._out("h0", (B, 147)), self._out("p0", (B, self.A))
        _lib.check(self.lib.smz_vision_initial_record(C.byref(self.desc), _ptr(self.weights), _ptr(obs),
                                                      None if record is None else _ptr(record), _ptr(hidden),
                                                      _ptr(policy), B, _stream(self.device)))
        return hidden, policy

    def recurrent(self, engine):
        ph = engine.parent_hidden
        B = ph.shape[0]
        hidden, reward, policy, value = self._round_out(B)         # (S is 147 here: the 3x7x7 hidden state)
        _lib.check(self.lib.smz_vision_recurrent(C.byref(self.desc), _ptr(self.weights), _ptr(ph), ph.stride(0),
                                                 _ptr(engine.last_action), _ptr(engine.branch), _ptr(hidden), _ptr(reward),
                                                 _ptr(policy), _ptr(value), B, _stream(self.device)))
        return hidden, reward, policy, value


def _lstm_trunk(seq):
    """(Linear, nn.LSTM, extract_tensor) -> (W_lin [H,in], b_lin [H], [(W_ih [4O,K], b_ih, b_hh) per layer]), float32."""
    lin, lstm = seq[0], seq[1]
    if not isinstance(lin, torch.nn.Linear) or not isinstance(lstm, torch.nn.LSTM):
        raise ValueError("not an lstm_model trunk (Linear, LSTM, extract_tensor)")
    if not lstm.bias or lstm.bidirectional or getattr(lstm, "proj_size", 0) or lin.bias is None:
        raise ValueError("lstm_model trunks are unidirectional LSTMs with biases and no projection")
    t = lambda x: x.detach().float()
    layers = [(t(getattr(lstm, f"weight_ih_l{l}")), t(getattr(lstm, f"bias_ih_l{l}")), t(getattr(lstm, f"bias_hh_l{l}")))
              for l in range(lstm.num_layers)]
    return t(lin.weight), t(lin.bias), layers


def _unwrap(m):
    return m.module if isinstance(m, torch.nn.DataParallel) else m


def lstm_trunks_from_modules(representation, prediction, afterstate_prediction, afterstate_dynamics, dynamics):
    """The seven recurrent trunks in smz_lstm_desc order + the representation Linear, from modules with the reference's
    attributes (compat_lstm.py)."""
    rep, pre, apr, ady, dyn = (_unwrap(m) for m in (representation, prediction, afterstate_prediction, afterstate_dynamics,
                                                     dynamics))
    trunks = [_lstm_trunk(s) for s in (dyn.reward, dyn.next_state_normalized, ady.next_state_normalized, pre.policy,
                                       pre.value, apr.policy, apr.value)]
    if len({len(t[2]) for t in trunks}) != 1:
        raise ValueError("lstm_model trunks with different numbers of layers")
    return trunks, (rep.state_norm.weight.detach().float(), rep.state_norm.bias.detach().float())


class LstmTorchHeads(Heads):
    """`lstm_model` heads (compat_lstm.py) on torch-ROCm ops + the HIP softmax / support-decode epilogues.

    The reference calls every head with batch 1: one length-1 sequence from h0 = c0 = 0.  Here every tree is such a
    sequence of its own (seq 1, batch B), which is what nn.LSTM computes for a [1, B, H] input: per layer
    gates = W_ih x + b_ih + b_hh (W_hh multiplies h0 = 0), c = sigmoid(i) tanh(g) (f multiplies c0 = 0),
    h = sigmoid(o) tanh(c).  The cell is written out with plain ops instead of calling the LSTM module so that the
    step-wise search stays capturable in one graph (static shapes, no library RNN descriptors or workspaces).  Both
    pairs of networks run for every tree and the branch flag selects, as in ModuleHeads."""
    wants_mlp_input, wants_parent_hidden = True, False

    def __init__(self, representation, prediction, afterstate_prediction, afterstate_dynamics, dynamics, num_actions,
                 support_size, device):
        super().__init__(device)
        trunks, rep = lstm_trunks_from_modules(representation, prediction, afterstate_prediction, afterstate_dynamics,
                                               dynamics)
        mv = lambda x: x.to(self.device).contiguous()
        self.trunks = [(mv(w), mv(b), [(mv(wi), mv(bi), mv(bh)) for wi, bi, bh in layers]) for w, b, layers in trunks]
        self.rep = (mv(rep[0]), mv(rep[1]))
        self.A, self.S = int(num_actions), int(support_size)

    @staticmethod
    def _scale(x):
        lo = x.amin(dim=1, keepdim=True)
        span = x.amax(dim=1, keepdim=True) - lo
        return (x - lo) / torch.where(span < 1e-5, span + 1e-5, span)

    def _trunk(self, t, x):
        w, b, layers = self.trunks[t]
        h = F.linear(x, w, b)
        for wi, bi, bh in layers:
            i, _, g, o = (F.linear(h, wi, bi) + bh).chunk(4, 1)
            h = torch.sigmoid(o) * torch.tanh(torch.sigmoid(i) * torch.tanh(g))
        return h

    @torch.no_grad()
    def initial(self, obs):
        B = obs.shape[0]
        hidden = self._scale(F.linear(obs, *self.rep)).contiguous()
        logits = self._trunk(3, hidden).contiguous()
        policy = self._out("p0", (B, self.A))
        _lib.check(self.lib.smz_policy_softmax(_ptr(logits), self.A, _ptr(policy), B, _stream(self.device)))
        return hidden, policy

    @torch.no_grad()
    def recurrent(self, engine):
        x, branch = engine.mlp_input, engine.branch
        B = x.shape[0]
        m = branch.bool()
        rl = self._trunk(0, x).contiguous()
        hidden = torch.where(m[:, None], self._scale(self._trunk(1, x)), self._scale(self._trunk(2, x))).contiguous()
        rdec = self._out("rdec", (B,))
        _lib.check(self.lib.smz_support_decode(_ptr(rl), self.S, _ptr(rdec), B, _stream(self.device)))
        reward = torch.where(m, rdec, torch.zeros_like(rdec)).contiguous()
        pl = torch.where(m[:, None], self._trunk(3, hidden), self._trunk(5, hidden)).contiguous()
        vl = torch.where(m[:, None], self._trunk(4, hidden), self._trunk(6, hidden)).contiguous()
        policy, value = self._out("p", (B, self.A)), self._out("v", (B,))
        _lib.check(self.lib.smz_policy_softmax(_ptr(pl), self.A, _ptr(policy), B, _stream(self.device)))
        _lib.check(self.lib.smz_support_decode(_ptr(vl), self.S, _ptr(value), B, _stream(self.device)))
        return hidden, reward, policy, value


class HipLstmHeads(Heads):
    """`lstm_model` heads evaluated by hand-written HIP kernels (smz_lstm_initial / smz_lstm_recurrent, csrc/smz_lstm.hip):
    the seven recurrent trunks packed once into the LDS layout of smz_lstm_desc (include/smz.h), each trunk's input Linear
    folded into its first LSTM layer on the host (float64 products, rounded once), forget gates and W_hh dropped (zero
    state).  Raises ValueError outside smz_lstm_layout's limits (use LstmTorchHeads then): obs <= 4096, A <= 64, 1 <= L <= 4, and
    the seven trunks plus four waves of scratch within 160 KB of LDS, which caps S at 48 -- (obs 9, A 4, S 48, L 1) is the last
    shape that fits (159,712 B); (9, 4, 49, 1) needs 175,024 B and (4, 2, 31, 3) 197,616 B."""
    wants_mlp_input, wants_parent_hidden = True, False
    single_launch = "lstm"

    def __init__(self, representation, prediction, afterstate_prediction, afterstate_dynamics, dynamics, num_actions,
                 support_size, device):
        import numpy as np
        super().__init__(device)
        trunks, (rep_w, rep_b) = lstm_trunks_from_modules(representation, prediction, afterstate_prediction,
                                                          afterstate_dynamics, dynamics)
        self.A, self.S = int(num_actions), int(support_size)
        self.obs, self.L = int(rep_w.shape[1]), len(trunks[0][2])
        d = _lib.LstmDesc(self.obs, self.A, self.S, self.L)
        if self.lib.smz_lstm_layout(C.byref(d)) != 0:
            # (lds_bytes stays 0 when a dimension is outside the limits: the layout returns before it sizes anything)
            needs = f", needs {d.lds_bytes} B" if d.lds_bytes > 0 else ""
            raise ValueError("lstm heads outside the HIP kernel's limits (obs <= 4096, A <= 64, 1 <= L <= 4, trunks + scratch "
                             f"within 160 KB of LDS, which caps S at 48; this net: obs {self.obs}, A {self.A}, S {self.S}, "
                             f"L {self.L}{needs})")
        self.desc = d
        buf = np.zeros(d.total_floats, np.float32)

        def put(idx, W, b):
            """W [G, K] (torch layout) -> input-major, 4-way interleaved, row width G; b [G]."""
            img = interleave(np.asarray(W, np.float32).T, len(b), 4)
            buf[d.off[idx]:d.off[idx] + img.size] = img
            buf[d.off[idx + 1]:d.off[idx + 1] + len(b)] = np.asarray(b, np.float32)

        f64 = lambda x: x.cpu().double().numpy()
        for t, (w, b, layers) in enumerate(trunks):
            O = layers[0][0].shape[0] // 4
            keep = np.r_[0:O, 2 * O:4 * O]                     # gates i, g, o (f multiplies c0 = 0)
            for l, (wi, bi, bh) in enumerate(layers):
                wi, bi, bh = f64(wi)[keep], f64(bi)[keep], f64(bh)[keep]
                if l == 0:      # no activation between the Linear and the first layer: fold it in
                    W, bias = wi @ f64(w), wi @ f64(b) + bi + bh
                else:
                    W, bias = wi, bi + bh
                put(2 * (t * _lib.LstmDesc.MAX_LAYERS + l), W, bias)
        put(_lib.LstmDesc.REP, rep_w.cpu().numpy(), rep_b.cpu().numpy())
        self.weights = torch.from_numpy(buf).to(self.device)

    def initial(self, obs):
        B = obs.shape[0]
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.obs
        hidden, policy = self._out("h0", (B, self.S)), self._out("p0", (B, self.A))
        _lib.check(self.lib.smz_lstm_initial(C.byref(self.desc), _ptr(self.weights), _ptr(obs), _ptr(hidden),
                                             _ptr(policy), B, _stream(self.device)))
        return hidden, policy

    def recurrent(self, engine):
        x, branch = engine.mlp_input, engine.branch
        B = x.shape[0]
        assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == self.S + self.A
        hidden, reward, policy, value = self._round_out(B)
        _lib.check(self.lib.smz_lstm_recurrent(C.byref(self.desc), _ptr(self.weights), _ptr(x), _ptr(branch),
                                               _ptr(hidden), _ptr(reward), _ptr(policy), _ptr(value), B,
                                               _stream(self.device)))
        return hidden, reward, policy, value


class ModuleHeads(Heads):
    """Heads given as five torch modules with the reference's signatures:
         representation(obs) -> hidden                                   (already scaled)
         prediction(h), afterstate_prediction(h) -> (policy_logits, value_logits)
         afterstate_dynamics(h, action_encoding) -> hidden
         dynamics(h, action_encoding) -> (reward_logits, hidden)
       `encode_action(last_action[B] int64, hidden) -> tensor` builds the action input (one-hot for vector
       observations, constant plane (a+1)/A for RGB: muzero_model.py:496-523)."""

    wants_mlp_input, wants_parent_hidden = False, True

    def __init__(self, representation, prediction, afterstate_prediction, afterstate_dynamics, dynamics, num_actions,
                 support_size, device, is_rgb=False):
        super().__init__(device)
        self.rep, self.pre, self.apr, self.ady, self.dyn = (m.to(self.device).eval() for m in (
            representation, prediction, afterstate_prediction, afterstate_dynamics, dynamics))
        self.A, self.Ssup, self.is_rgb = int(num_actions), int(support_size), bool(is_rgb)

    def encode_action(self, action, hidden):
        if not self.is_rgb:
            return F.one_hot(action.long(), self.A).to(hidden.dtype)
        plane = (action.to(hidden.dtype) + 1) / self.A
        return plane.view(-1, 1, 1, 1).expand(-1, 1, hidden.shape[2], hidden.shape[3]).contiguous()

    @torch.no_grad()
    def initial(self, obs):
        hidden = self.rep(obs)
        self.hidden_shape = tuple(hidden.shape[1:])
        logits, _ = self.pre(hidden)
        B = obs.shape[0]
        policy = self._out("p0", (B, self.A))
        logits = logits.float().contiguous()
        _lib.check(self.lib.smz_policy_softmax(_ptr(logits), self.A, _ptr(policy), B, _stream(self.device)))
        return hidden.reshape(B, -1).float().contiguous(), policy

    @torch.no_grad()
    def recurrent(self, engine):
        B = engine.B
        h = engine.parent_hidden[:, :engine.S].reshape((B,) + self.hidden_shape)
        enc = self.encode_action(engine.last_action, h)
        reward_logits, s_dyn = self.dyn(h, enc)
        s_aft = self.ady(h, enc)
        m = engine.branch.bool()
        hidden = torch.where(m.view((B,) + (1,) * (s_dyn.dim() - 1)), s_dyn, s_aft).contiguous()
        rl = reward_logits.float().contiguous()
        rdec = self._out("rdec", (B,))
        _lib.check(self.lib.smz_support_decode(_ptr(rl), self.Ssup, _ptr(rdec), B, _stream(self.device)))
        reward = torch.where(m, rdec, torch.zeros_like(rdec))
        pp, vp = self.pre(hidden)
        pa, va = self.apr(hidden)
        pp, vp, pa, va = (t.float().contiguous() for t in (pp, vp, pa, va))
        policy = self._out("p", (B, self.A))
        value = self._out("v", (B,))
        # policy rows (A wide) and value rows (S wide) have different strides: one epilogue call per width
        _lib.check(self.lib.smz_policy_softmax(_ptr(torch.where(m[:, None], pp, pa).contiguous()), self.A, _ptr(policy),
                                               B, _stream(self.device)))
        _lib.check(self.lib.smz_support_decode(_ptr(torch.where(m[:, None], vp, va).contiguous()), self.Ssup,
                                               _ptr(value), B, _stream(self.device)))
        return hidden.reshape(B, -1).float().contiguous(), reward.contiguous(), policy, value
