"""smz_mlp_initial_wide / smz_mlp_initial_large (csrc/smz_mlp_root.hip): declared alike by the header, the library and the
ctypes binding; the refusals the launcher makes on the host before any HIP call; the packed images of HipMlpTileHeads and
HipMlpLargeHeads evaluated in float64 through the kernel's addresses; the Python layers around the opt-in `hip_root`; and the
kernels' resource metadata (no scratch memory, no spilled vector registers: the code object's metadata block, no disassembly
is read).  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_mlp_large_abi import CSRC, FLAGS, HIPCC, OP, ROOT, M_PRE_IN, M_PRE_MID, M_PRE_OUT, M_REP_IN, M_REP_MID, M_REP_OUT, _binding, _pkg, _r8

ENTRY_POINTS = ("smz_mlp_initial_wide", "smz_mlp_initial_large")
WIDE, LARGE = (9, 3, 5, 7, 2), (9, 129, 5, 7, 2)


def _host_lib():
    so = os.path.join(ROOT, "stochastic-muzero_amd", "libsmz.so")
    if not os.path.exists(so):
        pytest.fail("libsmz.so is not built (python __graft_entry__.py build)")
    lib = C.CDLL(so)
    b = _binding()
    for name in ENTRY_POINTS + ("smz_mlp_layout_wide", "smz_mlp_layout_large"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = b.SIGNATURES[name]
    return lib, b


def test_header_binding_and_library_declare_the_root_entry_points():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    lib, b = _host_lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\nint %s\s*\(const smz_mlp_desc \*desc, const float \*weights_dev, const float \*obs_dev,\s+"
                         r"float \*hidden_out_dev,\s+float \*policy_out_dev, int B, smz_stream stream\);" % name, h), name
        res, args = b.SIGNATURES[name]
        assert res is C.c_int and len(args) == 7 and args[0]._type_ is b.MlpDesc and args[5] is C.c_int
        assert args == b.SIGNATURES["smz_mlp_initial"][1]
        assert hasattr(lib, name), name
    assert "present and unused" not in h


def test_the_launchers_refuse_on_the_host_before_any_hip_call():
    """Null pointers and B = 0 -> SMZ_ERR_INVALID; a wide descriptor handed to _large and the reverse -> SMZ_ERR_INVALID; a
    descriptor that is not its layout's -> SMZ_ERR_INVALID; obs = 1025 -> SMZ_ERR_TOO_LARGE.  The device pointers are dummies:
    every one of these calls returns before it would touch them (no GPU on this side of the suite)."""
    lib, b = _host_lib()
    dw, dl = b.MlpDesc(*WIDE), b.MlpDesc(*LARGE)
    assert lib.smz_mlp_layout_wide(C.byref(dw)) == 0 and lib.smz_mlp_layout_large(C.byref(dl)) == 0
    dummy = C.c_void_p(4096)
    for fn, d, other in ((lib.smz_mlp_initial_wide, dw, dl), (lib.smz_mlp_initial_large, dl, dw)):
        args = [C.byref(d), dummy, dummy, dummy, dummy, 8, None]
        for i in range(5):
            assert fn(*[None if j == i else x for j, x in enumerate(args)]) == b.SMZ_ERR_INVALID, i
        assert fn(*args[:5], 0, None) == b.SMZ_ERR_INVALID and fn(*args[:5], -3, None) == b.SMZ_ERR_INVALID
        assert fn(C.byref(other), *args[1:]) == b.SMZ_ERR_INVALID
        bad = b.MlpDesc.from_buffer_copy(d)
        bad.total_floats += 128
        assert fn(C.byref(bad), *args[1:]) == b.SMZ_ERR_INVALID
        bad = b.MlpDesc.from_buffer_copy(d)
        bad.off[M_REP_OUT] += 128
        assert fn(C.byref(bad), *args[1:]) == b.SMZ_ERR_INVALID
    # the same shape in the other layout (A + S <= 128: both layouts accept it, the images differ)
    both_w, both_l = b.MlpDesc(*WIDE), b.MlpDesc(*WIDE)
    assert lib.smz_mlp_layout_wide(C.byref(both_w)) == 0 and lib.smz_mlp_layout_large(C.byref(both_l)) == 0
    assert lib.smz_mlp_initial_wide(C.byref(both_l), dummy, dummy, dummy, dummy, 8, None) == b.SMZ_ERR_INVALID
    assert lib.smz_mlp_initial_large(C.byref(both_w), dummy, dummy, dummy, dummy, 8, None) == b.SMZ_ERR_INVALID
    for fn, layout, shape in ((lib.smz_mlp_initial_wide, lib.smz_mlp_layout_wide, (1025, 3, 5, 7, 2)),
                              (lib.smz_mlp_initial_large, lib.smz_mlp_layout_large, (1025, 129, 5, 7, 2))):
        d = b.MlpDesc(*shape)
        assert layout(C.byref(d)) == 0
        assert fn(C.byref(d), dummy, dummy, dummy, dummy, 8, None) == b.SMZ_ERR_TOO_LARGE, shape


def _arrays(model):
    model_mod = _pkg("model")
    return {k: np.asarray(v) for k, v in model_mod.mlp_arrays_from_modules(
        model.representation_function, model.prediction_function, model.afterstate_prediction_function,
        model.afterstate_dynamics_function, model.dynamics_function).items()}


def _wide_image(w, shape):
    """The packing of HipMlpTileHeads.__init__ itself: the constructor run on the CPU device (nothing is launched)."""
    heads = _pkg("heads").HipMlpTileHeads(w, dict(zip(("obs", "A", "S", "H", "L"), shape)), "cpu")
    return heads.packed.numpy(), heads.wide_desc


@pytest.mark.parametrize("shape", [WIDE, LARGE], ids=["wide", "large"])
def test_the_image_read_with_the_root_kernels_addresses_gives_the_restatements_outputs(shape):
    """Fresh nets (9,3,5,7,2) wide and (9,129,5,7,2) large, representation scaled too: the packed image evaluated in float64
    numpy through the address arithmetic of csrc/smz_mlp_root.hip -- rep_in in 8-input groups (obs = 9: a second group holding
    one input), the trunk, rep_out, the scaling, pre_in, the trunk, the policy columns (wide: the first A of [policy | value];
    large: panels with one bias vector per panel) -- on 64 random rows: Restatement.initial's hidden rows and policies to 1e-6
    (float32 weights on both sides; the figure of tests/test_mlp_large_abi.py for the same kind of check)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import mlp_reference as mr
    heads_mod, lib_mod = _pkg("heads"), _pkg("_lib")
    obs, A, S, H, L = shape
    large = shape == LARGE
    model = mr.fresh_net(*shape, seed=8, gain=4)
    with torch.no_grad():
        for p in model.representation_function.parameters():
            p.mul_(4.0)
    w = _arrays(model)
    d = lib_mod.MlpDesc(*shape)
    lib = lib_mod.load()
    if large:
        assert lib.smz_mlp_layout_large(C.byref(d)) == 0
        img = heads_mod.HipMlpLargeHeads.pack(w, d).astype(np.float64)
    else:
        img, d = _wide_image(w, shape)
        img = img.astype(np.float64)
    assert img.size == d.total_floats

    def layer(base, bias, x, K8):
        k = np.arange(8 * K8)
        o = np.arange(OP)
        return img[bias + o] + (x[k, None] * img[base + ((k[:, None] // 4) * OP + o[None, :]) * 4 + k[:, None] % 4]).sum(0)

    elu = lambda v: np.where(v > 0, v, np.exp(np.minimum(v, 0)) - 1)
    pad = lambda v, n: np.concatenate([v, np.zeros(n - v.size)])
    g = torch.Generator().manual_seed(10)
    rows = 64
    o = torch.randn(rows, obs, generator=g)
    want = mr.Restatement(model).initial(o)
    K8o, K8s, K8h, P = _r8(obs) // 8, _r8(S) // 8, _r8(H) // 8, (A + OP - 1) // OP
    assert K8o == 2
    off = lambda m: (d.off[m], d.off[15 + m])
    (r_in, rb_in), (r_mid, rb_mid), (r_out, rb_out) = off(M_REP_IN), off(M_REP_MID), off(M_REP_OUT)
    (p_in, pb_in), (p_mid, pb_mid), (p_out, pb_out) = off(M_PRE_IN), off(M_PRE_MID), off(M_PRE_OUT)
    for i in range(rows):
        t = pad(elu(layer(r_in, rb_in, pad(o[i].double().numpy(), 8 * K8o), K8o)[:H]), 8 * K8h)
        for _ in range(L):
            t = pad(elu(layer(r_mid, rb_mid, t, K8h)[:H]), 8 * K8h)
        state = layer(r_out, rb_out, t, K8h)[:S]
        span = state.max() - state.min()
        hid = (state - state.min()) / (span + 1e-5 if span < 1e-5 else span)
        np.testing.assert_allclose(hid, want["root_hidden"][i].numpy(), rtol=0, atol=1e-6)
        t = pad(elu(layer(p_in, pb_in, pad(hid, 8 * K8s), K8s)[:H]), 8 * K8h)
        for _ in range(L):
            t = pad(elu(layer(p_mid, pb_mid, t, K8h)[:H]), 8 * K8h)
        if large:
            logits = np.concatenate([layer(p_out + p * 8 * K8h * OP, pb_out + p * OP, t, K8h)[:min(OP, A - p * OP)] for p in range(P)])
        else:
            logits = layer(p_out, pb_out, t, K8h)[:A]
        e = np.exp(logits - logits.max())
        np.testing.assert_allclose(e / e.sum(), want["root_policy"][i].numpy(), rtol=0, atol=1e-6)


def test_python_layers_around_hip_root():
    """Muzero.hip_root is False and heads(hip_root=None) resolves to it; the flag separates the cache keys and leaves the keys
    without it as they were; the CLI sets it from "hip_root_evaluation", keeps the key away from BatchedMCTS and leaves the
    model alone without it; both head classes take hip_root and refuse obs > 1024 with it, naming the limit."""
    import inspect
    sys.path.insert(0, ROOT)
    model_mod, heads_mod = _pkg("model"), _pkg("heads")
    assert model_mod.Muzero.hip_root is False
    sig = inspect.signature(model_mod.Muzero.heads).parameters
    assert sig["hip_root"].default is None and list(sig)[1:] == ["device", "instance", "backend", "hip_root"]
    for cls in (heads_mod.HipMlpTileHeads, heads_mod.HipMlpLargeHeads):
        assert inspect.signature(cls.__init__).parameters["hip_root"].default is False
        assert cls.initial is heads_mod.FusedMlpHeads.initial
    m = model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=4, action_space_dimensions=40,
                         state_space_dimensions=8, hidden_layer_dimensions=16, number_of_hidden_layer=0, random_tag=0)
    assert m.hip_root is False
    plain = {("cpu", 0, b): b for b in ("auto", "large")}       # (what heads() would have built: only the key is looked up)
    m._heads = dict(plain)
    m._heads_version = {k: m.weights_version() for k in m._heads}
    assert m.heads("cpu") == "auto" and m.heads("cpu", hip_root=None) == "auto" and m.heads("cpu", hip_root=False) == "auto"
    assert m.heads("cpu", backend="large", hip_root=False) == "large"
    m.hip_root = True       # another key: nothing cached under it
    keys = lambda: set(m._heads)
    flagged = [k for k in (("cpu", 0, "auto"), ("cpu", 0, "large"))]
    m._heads.update({k + ("hip_root",): k[2] + "+root" for k in flagged})
    m._heads_version = {k: m.weights_version() for k in m._heads}
    assert m.heads("cpu") == "auto+root" and m.heads("cpu", backend="large") == "large+root"
    assert m.heads("cpu", hip_root=False) == "auto" and m.heads("cpu", backend="large", hip_root=True) == "large+root"
    m.hip_root = False
    assert m.heads("cpu") == "auto" and m.heads("cpu", hip_root=True) == "auto+root" and len(keys()) == 4
    assert model_mod.Muzero.hip_root is False

    import muzero_cli
    block = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
                 num_simulations=5, maxium_action_sample=2, number_of_player=1, custom_loop=None)
    with_key = dict(monte_carlo_tree_search=dict(block, hip_root_evaluation=True))
    assert "hip_root_evaluation" not in muzero_cli.mcts_kwargs(with_key)
    _pkg("mcts").BatchedMCTS(4, **muzero_cli.mcts_kwargs(with_key))
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block))) is m and m.hip_root is False
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block, hip_root_evaluation=False))).hip_root is False
    assert muzero_cli.set_heads_backend(m, with_key).hip_root is True and m.heads_backend == "auto"
    assert m.heads("cpu") == "auto+root" and model_mod.Muzero.hip_root is False
    for name in os.listdir(os.path.join(ROOT, "config")) if os.path.isdir(os.path.join(ROOT, "config")) else []:
        if name.endswith(".json"):
            with open(os.path.join(ROOT, "config", name)) as f:
                assert "hip_root_evaluation" not in f.read(), name

    assert issubclass(heads_mod.HipRootLimit, ValueError) and heads_mod.HIP_ROOT_MAX_OBS == 1024
    for entry in ENTRY_POINTS:
        heads_mod._check_hip_root(_pkg("_lib").load(), 1024, entry)
        with pytest.raises(ValueError, match="1024"):
            heads_mod._check_hip_root(_pkg("_lib").load(), 1025, entry)


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_root_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    """Every k_mlp_initial_* kernel of smz_mlp_root.hip (k_mlp_initial_wide, k_mlp_initial_large): private_segment_fixed_size ==
    0 and no VGPR spills.  Reported, not asserted: the register counts (this build: 244 and 252 vector registers, 64 of them
    accumulators)."""
    out = tmp_path / "mlp_root.s"
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), "smz_mlp_root.hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k:
            continue
        assert "k_mlp_initial_" in m.group(1) and "k_mlp_recurrent_large" not in m.group(1), m.group(1)
        seen[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
                            for f in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                      "agpr_count", "sgpr_count", "group_segment_fixed_size")}
    assert len(seen) == 2, sorted(seen)
    for n, f in sorted(seen.items()):
        print(n, f)
    assert not {n: f["private_segment_fixed_size"] for n, f in seen.items() if f["private_segment_fixed_size"]}
    assert not {n: f["vgpr_spill_count"] for n, f in seen.items() if f["vgpr_spill_count"]}
