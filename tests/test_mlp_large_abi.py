"""smz_mlp_layout_large / smz_mlp_recurrent_large (csrc/smz_mlp_large.hip): declared alike by the header, the library and the
ctypes binding; the host-side layout over its envelope; the packing of HipMlpLargeHeads read back element by element; the
Python layers around the opt-in backend; and the kernel's resource metadata (no scratch memory, no spilled vector registers:
the code object's metadata block, no disassembly is read).  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stochastic-muzero_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the library's own flags (csrc/Makefile)
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-function", "-Wno-unused-variable",
         "-Wno-unused-const-variable", "-S", "--cuda-device-only"]
ENTRY_POINTS = ("smz_mlp_layout_large", "smz_mlp_recurrent_large")
# (obs, A, S, H, L): the shapes of tests/test_gpu_mlp_large_heads.py
SHAPES = [(1, 1, 1, 1, 0), (3, 2, 5, 7, 2), (7, 3, 8, 8, 0), (4, 100, 29, 64, 0), (4, 128, 8, 16, 1), (4, 129, 8, 16, 1),
          (4, 362, 32, 64, 1), (4, 1000, 16, 64, 1), (5, 1024, 64, 128, 4)]
OP = 128
(M_DYN_IN, M_ADY_IN, M_DYN_MID, M_ADY_MID, M_DYN_OUT, M_ADY_OUT, M_PRE_IN, M_APR_IN, M_PRE_MID, M_APR_MID, M_PRE_OUT, M_APR_OUT,
 M_REP_IN, M_REP_MID, M_REP_OUT) = range(15)


def _binding():
    import importlib.util
    spec = importlib.util.spec_from_file_location("smz_lib_only", os.path.join(ROOT, "stochastic-muzero_amd", "_lib.py"))
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    return lib


def _host_lib():
    so = os.path.join(ROOT, "stochastic-muzero_amd", "libsmz.so")
    if not os.path.exists(so):
        pytest.fail("libsmz.so is not built (python __graft_entry__.py build)")
    lib = C.CDLL(so)
    b = _binding()
    lib.smz_mlp_layout_large.restype, lib.smz_mlp_layout_large.argtypes = b.SIGNATURES["smz_mlp_layout_large"]
    return lib, b


def _pkg(name):
    sys.path.insert(0, ROOT)
    import stochastic_muzero_amd  # noqa: F401
    from importlib import import_module
    return import_module("stochastic-muzero_amd." + name)


def _r8(k):
    return (k + 7) & ~7


def _pieces(shape):
    """Rows of 128 floats of every matrix, and bias vectors of 128 floats per matrix, as include/smz.h documents them."""
    obs, A, S, H, L = shape
    mid, pan = (_r8(H) if L > 0 else 0), (A + OP - 1) // OP + 1
    rows = [_r8(S) + A] * 2 + [mid] * 2 + [_r8(H)] * 2 + [_r8(S)] * 2 + [mid] * 2 + [pan * _r8(H)] * 2 + [_r8(obs), mid, _r8(H)]
    biases = [pan if m in (M_PRE_OUT, M_APR_OUT) else 1 for m in range(15)]
    return rows, biases


def test_header_and_binding_declare_the_large_entry_points():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"\nint smz_mlp_layout_large\(smz_mlp_desc \*desc\);", h)
    assert re.search(r"\nint smz_mlp_recurrent_large\(const smz_mlp_desc \*desc, const float \*weights_dev, "
                     r"const float \*parent_hidden_dev,\s+const int32_t \*last_action_dev, const uint8_t \*branch_dev, "
                     r"float \*hidden_out_dev,\s+float \*reward_out_dev, float \*policy_out_dev, float \*value_out_dev, int B, "
                     r"smz_stream stream\);", h)
    lib = _binding()
    assert len(lib.SIGNATURES["smz_mlp_layout_large"][1]) == 1 and len(lib.SIGNATURES["smz_mlp_recurrent_large"][1]) == 11
    for name in ENTRY_POINTS:
        assert lib.SIGNATURES[name][1][0]._type_ is lib.MlpDesc
    assert lib.SIGNATURES["smz_mlp_recurrent_large"][1][9] is C.c_int


def test_the_library_exports_the_large_entry_points():
    lib, _ = _host_lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_accepts_the_envelope_and_sums_to_the_documented_pieces(shape):
    lib, b = _host_lib()
    d = b.MlpDesc(*shape)
    assert lib.smz_mlp_layout_large(C.byref(d)) == 0 and d.OP == OP
    rows, biases = _pieces(shape)
    off = 0
    for m in range(15):
        assert d.off[m] == off and off % 4 == 0, m            # (floats: 16-byte aligned)
        off += rows[m] * OP
    for m in range(15):
        assert d.off[15 + m] == off and off % 4 == 0, m
        off += biases[m] * OP
    assert d.total_floats == off
    S, A = shape[2], shape[1]
    for m in (M_DYN_IN, M_ADY_IN):                            # the action table behind the hidden part
        assert (d.off[m] + _r8(S) * OP) % 4 == 0 and d.off[m] + (_r8(S) + A) * OP == d.off[m + 1]
    assert d.off[M_ADY_IN] + (_r8(S) + A) * OP <= d.off[15] < d.total_floats      # a table is never the image's last piece


def test_layout_refuses_what_is_outside_the_envelope():
    lib, b = _host_lib()
    for shape in [(4, 1025, 8, 16, 0), (4, 2, 65, 64, 0), (4, 2, 31, 129, 0)]:
        assert lib.smz_mlp_layout_large(C.byref(b.MlpDesc(*shape))) == b.SMZ_ERR_TOO_LARGE, shape
    for shape in [(4, 0, 8, 16, 0), (0, 2, 8, 16, 0), (4, 2, 0, 16, 0), (4, 2, 8, 0, 0), (4, 2, 8, 16, -1)]:
        assert lib.smz_mlp_layout_large(C.byref(b.MlpDesc(*shape))) == b.SMZ_ERR_INVALID, shape
    assert lib.smz_mlp_layout_large(None) == b.SMZ_ERR_INVALID
    # (the older layouts keep refusing what they refused)
    lib.smz_mlp_layout_wide.restype, lib.smz_mlp_layout_wide.argtypes = b.SIGNATURES["smz_mlp_layout_wide"]
    assert lib.smz_mlp_layout_wide(C.byref(b.MlpDesc(4, 100, 29, 64, 0))) == b.SMZ_ERR_TOO_LARGE


def test_packing_round_trip():
    """The packed image of a fresh (4,129,5,7,2) net read back with the formulas of include/smz.h: every element of every
    matrix the kernel reads (hidden parts, action-table rows, panel columns, value columns, biases) against
    mlp_arrays_from_modules; padding inputs, padding columns and everything else in the image exactly 0."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mlp_reference as mr
    heads_mod, model_mod, lib_mod = _pkg("heads"), _pkg("model"), _pkg("_lib")
    shape = (4, 129, 5, 7, 2)
    obs, A, S, H, L = shape
    model = mr.fresh_net(*shape, seed=5, gain=4)
    w = {k: np.asarray(v) for k, v in model_mod.mlp_arrays_from_modules(
        model.representation_function, model.prediction_function, model.afterstate_prediction_function,
        model.afterstate_dynamics_function, model.dynamics_function).items()}
    d = lib_mod.MlpDesc(*shape)
    assert lib_mod.load().smz_mlp_layout_large(C.byref(d)) == 0
    img = heads_mod.HipMlpLargeHeads.pack(w, d)
    assert img.dtype == np.float32 and img.size == d.total_floats
    seen = np.zeros(img.size, bool)

    def wide(base, Wt):
        """Wt [K, O] input-major: element (k, o) at base + ((k / 4) * 128 + o) * 4 + k % 4."""
        K, O = Wt.shape
        for k in range(K):
            for o in range(O):
                i = base + ((k // 4) * OP + o) * 4 + k % 4
                assert img[i] == Wt[k, o], (base, k, o)
                seen[i] = True

    def vec(base, b):
        assert np.array_equal(img[base:base + b.size], b), base
        seen[base:base + b.size] = True

    for tag, m in (("dyn", M_DYN_IN), ("ady", M_ADY_IN)):
        Wt = w[tag + "_in_w"].T                               # [S + A, H]
        wide(d.off[m], Wt[:S])
        table = d.off[m] + _r8(S) * OP
        for a in range(A):                                    # (rows 0, 127, 128 among them)
            assert np.array_equal(img[table + a * OP:table + a * OP + H], Wt[S + a]), (tag, a)
            seen[table + a * OP:table + a * OP + H] = True
        vec(d.off[15 + m], w[tag + "_in_b"])
    for tag, m in (("pre", M_PRE_OUT), ("apr", M_APR_OUT)):
        pol, val = w[tag + "_pol_w"].T, w[tag + "_val_w"].T   # [H, A], [H, S]
        wide(d.off[m], pol[:, :128])                          # panel 0: columns 0 .. 127
        wide(d.off[m] + _r8(H) * OP, pol[:, 128:])            # panel 1: column 128
        wide(d.off[m] + 2 * _r8(H) * OP, val)                 # the value panel
        vec(d.off[15 + m], w[tag + "_pol_b"][:128])
        vec(d.off[15 + m] + OP, w[tag + "_pol_b"][128:])
        vec(d.off[15 + m] + 2 * OP, w[tag + "_val_b"])
    for m, parts in ((M_DYN_MID, ["dyn_mid"]), (M_ADY_MID, ["ady_mid"]), (M_DYN_OUT, ["dyn_rw", "dyn_st"]), (M_ADY_OUT, ["ady_st"]),
                     (M_PRE_IN, ["pre_in"]), (M_APR_IN, ["apr_in"]), (M_PRE_MID, ["pre_mid"]), (M_APR_MID, ["apr_mid"]),
                     (M_REP_IN, ["rep_in"]), (M_REP_MID, ["rep_mid"]), (M_REP_OUT, ["rep_out"])):
        wide(d.off[m], np.concatenate([w[p + "_w"] for p in parts], 0).T)
        vec(d.off[15 + m], np.concatenate([w[p + "_b"] for p in parts], 0))
    assert 0 < seen.sum() < img.size and (img[~seen] == 0).all()


# (layout entry point, name of the evaluator, its image, its descriptor, (obs, A, S, H, L), OP, K is padded to a multiple of):
# odd sizes that are no multiple of the padding, with hidden layers; the wide shape is one the LDS layout refuses (2 S > 64)
PLAIN_IMAGES = [("smz_mlp_layout", "HipMlpHeads", "weights", "desc", (5, 3, 5, 7, 2), 64, 4),
                ("smz_mlp_layout_wide", "HipMlpTileHeads", "packed", "wide_desc", (5, 3, 33, 70, 2), 128, 8)]


@pytest.mark.parametrize("entry,cls,image,desc,shape,op,pad", PLAIN_IMAGES, ids=[p[0] for p in PLAIN_IMAGES])
def test_lds_and_wide_packing_round_trip(entry, cls, image, desc, shape, op, pad):
    """The other two mlp_model images, as the evaluators built on the CPU device hold them, of a fresh net each: every weight at
    off[m] + ((k / 4) * OP + o) * 4 + k % 4 and every bias at off[15 + m] + o (include/smz.h) against mlp_arrays_from_modules,
    matrix by matrix in the documented order; K padded to 4 (LDS) or 8 (wide) inputs; everything else in the image exactly 0."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mlp_reference as mr
    heads_mod, model_mod = _pkg("heads"), _pkg("model")
    model = mr.fresh_net(*shape, seed=7, gain=4)
    w = {k: np.asarray(v) for k, v in model_mod.mlp_arrays_from_modules(
        model.representation_function, model.prediction_function, model.afterstate_prediction_function,
        model.afterstate_dynamics_function, model.dynamics_function).items()}
    obs, A, S, H, L = shape
    heads = getattr(heads_mod, cls)(w, dict(obs=obs, A=A, S=S, H=H, L=L), "cpu")
    d, img = getattr(heads, desc), getattr(heads, image).numpy()
    assert d.OP == op and img.dtype == np.float32 and img.size == d.total_floats
    seen = np.zeros(img.size, bool)
    mats = [["dyn_in"], ["ady_in"], ["dyn_mid"], ["ady_mid"], ["dyn_rw", "dyn_st"], ["ady_st"], ["pre_in"], ["apr_in"], ["pre_mid"],
            ["apr_mid"], ["pre_pol", "pre_val"], ["apr_pol", "apr_val"], ["rep_in"], ["rep_mid"], ["rep_out"]]
    shapes = [(S + A, H), (S + A, H), (H, H), (H, H), (H, 2 * S), (H, S), (S, H), (S, H), (H, H), (H, H), (H, A + S), (H, A + S),
              (obs, H), (H, H), (H, S)]
    for m, parts in enumerate(mats):
        Wt = np.concatenate([w[p + "_w"] for p in parts], 0).T            # [K, O]
        b = np.concatenate([w[p + "_b"] for p in parts], 0)
        K, O = Wt.shape
        assert (K, O) == shapes[m] and b.shape == (O,) and O <= op
        for k in range(K):
            for o in range(O):
                i = d.off[m] + ((k // 4) * op + o) * 4 + k % 4
                assert img[i] == Wt[k, o] and not seen[i], (m, k, o)
                seen[i] = True
        for o in range(O):
            i = d.off[15 + m] + o
            assert img[i] == b[o] and not seen[i], (m, o)
            seen[i] = True
        # the matrix's padded rows end where the next piece begins, or before
        nxt = min([x for x in list(d.off) + [d.total_floats] if x > d.off[m]])
        assert d.off[m] + (K + pad - 1) // pad * pad * op <= nxt, m
    assert 0 < seen.sum() < img.size and (img[~seen] == 0).all()


def test_the_image_read_with_the_kernels_addresses_gives_the_restatements_outputs():
    """The packed image of a fresh (4,129,5,7,2) net evaluated in float64 numpy through the address arithmetic of
    csrc/smz_mlp_large.hip -- hidden part + action-table row, 8-input groups, panels, one bias vector per panel -- on 64 rows
    of mixed branches: the float64 restatement's hidden rows, policies and logits to 1e-6 (float32 weights on both sides)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import mlp_reference as mr
    heads_mod, model_mod, lib_mod = _pkg("heads"), _pkg("model"), _pkg("_lib")
    shape = (4, 129, 5, 7, 2)
    obs, A, S, H, L = shape
    model = mr.fresh_net(*shape, seed=6, gain=4)
    w = model_mod.mlp_arrays_from_modules(model.representation_function, model.prediction_function,
                                          model.afterstate_prediction_function, model.afterstate_dynamics_function,
                                          model.dynamics_function)
    d = lib_mod.MlpDesc(*shape)
    assert lib_mod.load().smz_mlp_layout_large(C.byref(d)) == 0
    img = heads_mod.HipMlpLargeHeads.pack({k: np.asarray(v) for k, v in w.items()}, d).astype(np.float64)

    def layer(base, bias, x, K8):
        """x [8 K8] -> 128 outputs: sum_k x[k] * img[base + ((k / 4) * 128 + o) * 4 + k % 4] + img[bias + o]"""
        k = np.arange(8 * K8)
        o = np.arange(OP)
        return img[bias + o] + (x[k, None] * img[base + ((k[:, None] // 4) * OP + o[None, :]) * 4 + k[:, None] % 4]).sum(0)

    elu = lambda v: np.where(v > 0, v, np.exp(np.minimum(v, 0)) - 1)
    pad = lambda v, n: np.concatenate([v, np.zeros(n - v.size)])
    g = torch.Generator().manual_seed(9)
    rows = 64
    h = torch.rand(rows, S, generator=g)
    a = torch.randint(0, A, (rows,), generator=g)
    a[:4] = torch.tensor([0, 127, 128, A - 1])
    br = torch.randint(0, 2, (rows,), generator=g)
    want = mr.Restatement(model).recurrent(h, a, br)
    K8s, K8h, P = _r8(S) // 8, _r8(H) // 8, (A + OP - 1) // OP
    for i in range(rows):
        ady = int(br[i]) == 0
        off = lambda m: (d.off[m + (1 if ady else 0)], d.off[15 + m + (1 if ady else 0)])
        (w_in, b_in), (w_mid, b_mid), (w_out, b_out) = off(M_DYN_IN), off(M_DYN_MID), off(M_DYN_OUT)
        (p_in, pb_in), (p_mid, pb_mid), (p_out, pb_out) = off(M_PRE_IN), off(M_PRE_MID), off(M_PRE_OUT)
        y = layer(w_in, b_in, pad(h[i].double().numpy(), 8 * K8s), K8s)
        table = w_in + 8 * K8s * OP + int(a[i]) * OP
        y = y + img[table:table + OP]
        t = pad(elu(y[:H]), 8 * K8h)
        for _ in range(L):
            t = pad(elu(layer(w_mid, b_mid, t, K8h)[:H]), 8 * K8h)
        y = layer(w_out, b_out, t, K8h)
        state = y[:S] if ady else y[S:2 * S]
        span = state.max() - state.min()
        hid = (state - state.min()) / (span + 1e-5 if span < 1e-5 else span)
        np.testing.assert_allclose(hid, want["hidden"][i].numpy(), rtol=0, atol=1e-6)
        if not ady:
            np.testing.assert_allclose(y[:S], want["reward_logits"][i].numpy(), rtol=0, atol=1e-6)
        t = pad(elu(layer(p_in, pb_in, pad(hid, 8 * K8s), K8s)[:H]), 8 * K8h)
        for _ in range(L):
            t = pad(elu(layer(p_mid, pb_mid, t, K8h)[:H]), 8 * K8h)
        logits = np.concatenate([layer(p_out + p * 8 * K8h * OP, pb_out + p * OP, t, K8h)[:min(OP, A - p * OP)] for p in range(P)])
        e = np.exp(logits - logits.max())
        np.testing.assert_allclose(e / e.sum(), want["policy"][i].numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(layer(p_out + P * 8 * K8h * OP, pb_out + P * OP, t, K8h)[:S], want["value_logits"][i].numpy(),
                                   rtol=0, atol=1e-6)


def test_python_layers_around_the_backend():
    """Muzero.heads_backend defaults to "auto" and heads(backend=None) resolves to it; the CLI sets it from the config key and
    keeps the key away from BatchedMCTS; a config without the key leaves the model alone."""
    import inspect
    sys.path.insert(0, ROOT)
    model_mod, heads_mod = _pkg("model"), _pkg("heads")
    assert model_mod.Muzero.heads_backend == "auto"
    assert inspect.signature(model_mod.Muzero.heads).parameters["backend"].default is None
    assert issubclass(heads_mod.HipMlpLargeHeads, heads_mod.FusedMlpHeads)
    assert (heads_mod.HipMlpLargeHeads.wants_mlp_input, heads_mod.HipMlpLargeHeads.wants_parent_hidden) == (False, True)
    m = model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=4, action_space_dimensions=40,
                         state_space_dimensions=8, hidden_layer_dimensions=16, number_of_hidden_layer=0, random_tag=0)
    assert m.heads_backend == "auto"
    m._heads ={("cpu", 0, b): b for b in ("auto", "large")}      # (what heads() would have built: only the key is looked up)
    m._heads_version = {k: m.weights_version() for k in m._heads}
    assert m.heads("cpu") == "auto" and m.heads("cpu", backend=None) == "auto" and m.heads("cpu", backend="large") == "large"
    import muzero_cli
    block = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
                 num_simulations=5, maxium_action_sample=2, number_of_player=1, custom_loop=None)
    with_key = dict(monte_carlo_tree_search=dict(block, large_action_heads=True))
    assert "large_action_heads" not in muzero_cli.mcts_kwargs(with_key)
    _pkg("mcts").BatchedMCTS(4, **muzero_cli.mcts_kwargs(with_key))
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block))) is m and m.heads_backend == "auto"
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block, large_action_heads=False))).heads_backend == "auto"
    assert muzero_cli.set_heads_backend(m, with_key).heads_backend == "large"
    assert m.heads("cpu") == "large" and model_mod.Muzero.heads_backend == "auto"


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_large_kernel_uses_no_scratch_and_spills_no_vector_registers(tmp_path):
    """Every k_mlp_recurrent_large* kernel (the wavefront-per-tile one and the split one): private_segment_fixed_size == 0 and no
    VGPR spills.  Reported, not asserted: the register counts (this build: 240 and 236 vector registers, 64 of them
    accumulators: two wavefronts per SIMD)."""
    out = tmp_path / "mlp_large.s"
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), "smz_mlp_large.hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k or "k_mlp_recurrent_large" not in m.group(1):
            continue
        seen[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
                            for f in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                      "agpr_count", "sgpr_count", "group_segment_fixed_size")}
    assert len(seen) == 2 and any("large_split" in n for n in seen), sorted(seen)
    for n, f in sorted(seen.items()):
        print(n, f)
    assert not {n: f["private_segment_fixed_size"] for n, f in seen.items() if f["private_segment_fixed_size"]}
    assert not {n: f["vgpr_spill_count"] for n, f in seen.items() if f["vgpr_spill_count"]}
