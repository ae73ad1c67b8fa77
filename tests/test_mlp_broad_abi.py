"""smz_mlp_layout_broad / smz_mlp_recurrent_broad (csrc/smz_mlp_broad.hip): declared alike by the header, the library and the
ctypes binding; the host-side layout over its envelope; the packing of HipMlpBroadHeads read back element by element through
the formula of include/smz.h; the image evaluated through the kernel's address arithmetic; the Python layers around the opt-in
backend; and the kernel's resource metadata (no scratch memory, no spilled vector registers: the code object's metadata
block, no disassembly is read).  Nothing here needs a GPU."""
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
ENTRY_POINTS = ("smz_mlp_layout_broad", "smz_mlp_recurrent_broad")
# (obs, A, S, H, L): the shapes of tests/test_gpu_mlp_broad_heads.py
SHAPES = [(1, 1, 1, 1, 0), (3, 2, 5, 129, 1), (4, 2, 65, 64, 0), (4, 3, 129, 130, 2), (4, 2, 100, 384, 0), (4, 129, 8, 256, 1),
          (4, 1000, 16, 200, 1), (5, 1024, 256, 512, 4)]
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
    for name in ("smz_mlp_layout_broad", "smz_mlp_layout_large", "smz_mlp_layout_wide"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = b.SIGNATURES[name]
    return lib, b


def _pkg(name):
    sys.path.insert(0, ROOT)
    import stochastic_muzero_amd  # noqa: F401
    from importlib import import_module
    return import_module("stochastic-muzero_amd." + name)


def _r8(k):
    return (k + 7) & ~7


def _p(n):
    return (n + OP - 1) // OP


def _pieces(shape):
    """Rows of 128 floats of every matrix, and bias vectors of 128 floats per matrix, as include/smz.h documents them."""
    obs, A, S, H, L = shape
    ph, ps, pa = _p(H), _p(S), _p(A)
    mid, pmid = (ph * _r8(H), ph) if L > 0 else (0, 0)
    rows = [ph * _r8(S) + A * ph] * 2 + [mid] * 2 + [2 * ps * _r8(H), ps * _r8(H)] + [ph * _r8(S)] * 2 + [mid] * 2 + \
           [(pa + ps) * _r8(H)] * 2 + [ph * _r8(obs), mid, ps * _r8(H)]
    biases = [ph, ph, pmid, pmid, 2 * ps, ps, ph, ph, pmid, pmid, pa + ps, pa + ps, ph, pmid, ps]
    return rows, biases


def _weight(base, K, k, o):
    """include/smz.h: weight (k, o) of a panel matrix of K inputs at base."""
    return base + (o // OP) * _r8(K) * OP + ((k // 4) * OP + o % OP) * 4 + k % 4


def test_header_and_binding_declare_the_broad_entry_points():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"\nint smz_mlp_layout_broad\(smz_mlp_desc \*desc\);", h)
    assert re.search(r"\nint smz_mlp_recurrent_broad\(const smz_mlp_desc \*desc, const float \*weights_dev, "
                     r"const float \*parent_hidden_dev,\s+const int32_t \*last_action_dev, const uint8_t \*branch_dev, "
                     r"float \*hidden_out_dev,\s+float \*reward_out_dev, float \*policy_out_dev, float \*value_out_dev, int B, "
                     r"smz_stream stream\);", h)
    assert re.search(r"#define SMZ_ABI_VERSION 1\b", h)
    lib = _binding()
    assert len(lib.SIGNATURES["smz_mlp_layout_broad"][1]) == 1
    assert lib.SIGNATURES["smz_mlp_recurrent_broad"] == lib.SIGNATURES["smz_mlp_recurrent_large"]
    for name in ENTRY_POINTS:
        assert lib.SIGNATURES[name][1][0]._type_ is lib.MlpDesc


def test_the_library_exports_the_broad_entry_points():
    lib, _ = _host_lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_accepts_the_envelope_and_sums_to_the_documented_pieces(shape):
    lib, b = _host_lib()
    d = b.MlpDesc(*shape)
    assert lib.smz_mlp_layout_broad(C.byref(d)) == 0 and d.OP == OP
    rows, biases = _pieces(shape)
    off = 0
    for m in range(15):
        assert d.off[m] == off and off % 4 == 0, m            # (floats: 16-byte aligned)
        off += rows[m] * OP
    for m in range(15):
        assert d.off[15 + m] == off and off % 4 == 0, m
        off += biases[m] * OP
    assert d.total_floats == off
    _, A, S, H, _ = shape
    for m in (M_DYN_IN, M_ADY_IN):                            # the action table behind the hidden part's panels
        assert d.off[m] + (_p(H) * _r8(S) + A * _p(H)) * OP == d.off[m + 1]
    assert d.off[M_ADY_IN] + (_p(H) * _r8(S) + (A + 1) * _p(H)) * OP <= d.total_floats      # a table is never the image's last piece


def test_layout_refuses_what_is_outside_the_envelope():
    lib, b = _host_lib()
    for shape in [(4, 2, 8, 513, 0), (4, 2, 257, 64, 0), (4, 1025, 8, 16, 0)]:
        assert lib.smz_mlp_layout_broad(C.byref(b.MlpDesc(*shape))) == b.SMZ_ERR_TOO_LARGE, shape
    for shape in [(4, 0, 8, 16, 0), (0, 2, 8, 16, 0), (4, 2, 0, 16, 0), (4, 2, 8, 0, 0), (4, 2, 8, 16, -1), (4, -1, 8, 16, 0),
                  (4, 2, -8, 16, 0), (4, 2, 8, -16, 0), (-4, 2, 8, 16, 0)]:
        assert lib.smz_mlp_layout_broad(C.byref(b.MlpDesc(*shape))) == b.SMZ_ERR_INVALID, shape
    assert lib.smz_mlp_layout_broad(None) == b.SMZ_ERR_INVALID
    for shape in [(4, 2, 8, 512, 0), (4, 2, 256, 64, 0), (4, 1024, 8, 16, 0)]:      # (the limits themselves)
        assert lib.smz_mlp_layout_broad(C.byref(b.MlpDesc(*shape))) == 0, shape
    # (the older layouts keep refusing what they refused)
    for shape in [(4, 2, 65, 64, 0), (4, 2, 31, 129, 0)]:
        assert lib.smz_mlp_layout_wide(C.byref(b.MlpDesc(*shape))) == b.SMZ_ERR_TOO_LARGE, shape
        assert lib.smz_mlp_layout_large(C.byref(b.MlpDesc(*shape))) == b.SMZ_ERR_TOO_LARGE, shape


def _fresh(shape, seed):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mlp_reference as mr
    model_mod = _pkg("model")
    model = mr.fresh_net(*shape, seed=seed, gain=4)
    w = {k: np.asarray(v) for k, v in model_mod.mlp_arrays_from_modules(
        model.representation_function, model.prediction_function, model.afterstate_prediction_function,
        model.afterstate_dynamics_function, model.dynamics_function).items()}
    return model, w


def test_packing_round_trip():
    """The packed image of a fresh (4,129,130,131,2) net read back with the formula of include/smz.h: every weight of every
    matrix (hidden parts, action-table rows, the reward / state and policy / value column ranges in panels of their own) and
    every bias against mlp_arrays_from_modules; no element claimed twice; everything else in the image exactly 0."""
    heads_mod, lib_mod = _pkg("heads"), _pkg("_lib")
    shape = (4, 129, 130, 131, 2)
    obs, A, S, H, L = shape
    _, w = _fresh(shape, 5)
    d = lib_mod.MlpDesc(*shape)
    assert lib_mod.load().smz_mlp_layout_broad(C.byref(d)) == 0
    img = heads_mod.HipMlpBroadHeads.pack(w, d)
    assert img.dtype == np.float32 and img.size == d.total_floats
    seen = np.zeros(img.size, bool)

    def claim(idx, want, what):
        idx = np.asarray(idx).reshape(-1)
        assert not seen[idx].any() and np.unique(idx).size == idx.size, what
        assert np.array_equal(img[idx], np.asarray(want, np.float32).reshape(-1)), what
        seen[idx] = True

    def matrix(base, bias, W, b, what):
        """W [O, K] (torch layout), b [O]: a panel matrix at base, its biases at bias."""
        O, K = W.shape
        k, o = np.meshgrid(np.arange(K), np.arange(O), indexing="ij")
        claim(_weight(base, K, k, o), W.T, what)
        claim(bias + np.arange(O), b, what + " bias")
        return base + _p(O) * _r8(K) * OP, bias + _p(O) * OP

    for tag, m in (("dyn", M_DYN_IN), ("ady", M_ADY_IN)):
        W, b = w[tag + "_in_w"], w[tag + "_in_b"]             # [H, S + A]
        table, _ = matrix(d.off[m], d.off[15 + m], W[:, :S], b, tag + "_in")
        assert table == d.off[m] + _p(H) * _r8(S) * OP
        a, o = np.meshgrid(np.arange(A), np.arange(H), indexing="ij")      # (rows 0, 127, 128 among them)
        claim(table + a * OP * _p(H) + o, W[:, S:].T, tag + " table")
    at, bias = matrix(d.off[M_DYN_OUT], d.off[15 + M_DYN_OUT], w["dyn_rw_w"], w["dyn_rw_b"], "reward")
    assert (at, bias) == (d.off[M_DYN_OUT] + _p(S) * _r8(H) * OP, d.off[15 + M_DYN_OUT] + _p(S) * OP)
    matrix(at, bias, w["dyn_st_w"], w["dyn_st_b"], "state")
    for tag, m in (("pre", M_PRE_OUT), ("apr", M_APR_OUT)):
        at, bias = matrix(d.off[m], d.off[15 + m], w[tag + "_pol_w"], w[tag + "_pol_b"], tag + " policy")
        assert (at, bias) == (d.off[m] + _p(A) * _r8(H) * OP, d.off[15 + m] + _p(A) * OP)
        matrix(at, bias, w[tag + "_val_w"], w[tag + "_val_b"], tag + " value")
    for m, name in ((M_DYN_MID, "dyn_mid"), (M_ADY_MID, "ady_mid"), (M_ADY_OUT, "ady_st"), (M_PRE_IN, "pre_in"), (M_APR_IN, "apr_in"),
                    (M_PRE_MID, "pre_mid"), (M_APR_MID, "apr_mid"), (M_REP_IN, "rep_in"), (M_REP_MID, "rep_mid"), (M_REP_OUT, "rep_out")):
        matrix(d.off[m], d.off[15 + m], w[name + "_w"], w[name + "_b"], name)
    assert 0 < seen.sum() < img.size and (img[~seen] == 0).all()
    n_weights = sum(v.size for v in w.values())
    assert seen.sum() == n_weights


def test_the_image_read_with_the_kernels_addresses_gives_the_restatements_outputs():
    """The packed image of a fresh (4,129,130,131,2) net evaluated in float64 numpy through the address arithmetic of
    csrc/smz_mlp_broad_device.hpp -- 8-input groups, 128-column panels with a bias vector each, hidden part + action-table row,
    reward / state and policy / value panels -- on 64 rows of mixed branches with actions 0, 127, 128 and A - 1 among them:
    the float64 restatement's hidden rows, policies and logits to 1e-6 (float32 weights on both sides)."""
    import torch
    heads_mod, lib_mod = _pkg("heads"), _pkg("_lib")
    shape = (4, 129, 130, 131, 2)
    obs, A, S, H, L = shape
    model, w = _fresh(shape, 6)
    import mlp_reference as mr
    d = lib_mod.MlpDesc(*shape)
    assert lib_mod.load().smz_mlp_layout_broad(C.byref(d)) == 0
    img = heads_mod.HipMlpBroadHeads.pack(w, d).astype(np.float64)

    def panel(base, bias, x, K8):
        """wide_layer: x [8 K8] -> 128 outputs: sum_k x[k] * img[base + ((k / 4) * 128 + o) * 4 + k % 4] + img[bias + o]"""
        k = np.arange(8 * K8)
        o = np.arange(OP)
        return img[bias + o] + (x[k, None] * img[base + ((k[:, None] // 4) * OP + o[None, :]) * 4 + k[:, None] % 4]).sum(0)

    def layer(base, bias, x, K8, panels, first=0):
        """panels first .. first + panels - 1 of the matrix at base, one after the other"""
        return np.concatenate([panel(base + p * 8 * K8 * OP, bias + p * OP, x, K8) for p in range(first, first + panels)])

    elu = lambda v: np.where(v > 0, v, np.exp(np.minimum(v, 0)) - 1)
    pad = lambda v, n: np.concatenate([v, np.zeros(n - v.size)])
    g = torch.Generator().manual_seed(9)
    rows = 64
    h = torch.rand(rows, S, generator=g)
    a = torch.randint(0, A, (rows,), generator=g)
    a[:4] = torch.tensor([0, 127, 128, A - 1])
    br = torch.randint(0, 2, (rows,), generator=g)
    assert 0 < int(br.sum()) < rows
    want = mr.Restatement(model).recurrent(h, a, br)
    K8s, K8h, PH, PS, PA = _r8(S) // 8, _r8(H) // 8, _p(H), _p(S), _p(A)
    for i in range(rows):
        ady = int(br[i]) == 0
        off = lambda m: (d.off[m + (1 if ady else 0)], d.off[15 + m + (1 if ady else 0)])
        (w_in, b_in), (w_mid, b_mid), (w_out, b_out) = off(M_DYN_IN), off(M_DYN_MID), off(M_DYN_OUT)
        (p_in, pb_in), (p_mid, pb_mid), (p_out, pb_out) = off(M_PRE_IN), off(M_PRE_MID), off(M_PRE_OUT)
        y = layer(w_in, b_in, pad(h[i].double().numpy(), 8 * K8s), K8s, PH)
        table = w_in + PH * 8 * K8s * OP + int(a[i]) * PH * OP
        y = y + img[table:table + PH * OP]
        assert (y[H:] == 0).all()                             # (padding columns: the padding inputs of the next layer)
        t = elu(y)[:8 * K8h]
        for _ in range(L):
            t = elu(layer(w_mid, b_mid, t, K8h, PH))[:8 * K8h]
        if ady:
            state = layer(w_out, b_out, t, K8h, PS)[:S]
        else:
            np.testing.assert_allclose(layer(w_out, b_out, t, K8h, PS)[:S], want["reward_logits"][i].numpy(), rtol=0, atol=1e-6)
            state = layer(w_out, b_out, t, K8h, PS, first=PS)[:S]
        span = state.max() - state.min()
        hid = (state - state.min()) / (span + 1e-5 if span < 1e-5 else span)
        np.testing.assert_allclose(hid, want["hidden"][i].numpy(), rtol=0, atol=1e-6)
        t = elu(layer(p_in, pb_in, pad(hid, 8 * K8s), K8s, PH))[:8 * K8h]
        for _ in range(L):
            t = elu(layer(p_mid, pb_mid, t, K8h, PH))[:8 * K8h]
        logits = layer(p_out, pb_out, t, K8h, PA)[:A]
        e = np.exp(logits - logits.max())
        np.testing.assert_allclose(e / e.sum(), want["policy"][i].numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(layer(p_out, pb_out, t, K8h, PS, first=PA)[:S], want["value_logits"][i].numpy(), rtol=0, atol=1e-6)


def test_python_layers_around_the_backend():
    """Muzero.heads_backend stays "auto"; the CLI sets "broad" from the config key "broad_heads" and keeps the key away from
    BatchedMCTS; both backend keys together raise; a (4,2,16,256,1) model still gets FusedMlpHeads from "auto"."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mlp_reference as mr
    model_mod, heads_mod = _pkg("model"), _pkg("heads")
    assert model_mod.Muzero.heads_backend == "auto"
    cls = heads_mod.HipMlpBroadHeads
    assert issubclass(cls, heads_mod.FusedMlpHeads) and (cls.wants_mlp_input, cls.wants_parent_hidden) == (False, True)
    assert cls.single_launch is None and cls.initial is heads_mod.FusedMlpHeads.initial
    assert isinstance(cls.__dict__["pack"], staticmethod)
    m = model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=4, action_space_dimensions=40,
                         state_space_dimensions=8, hidden_layer_dimensions=16, number_of_hidden_layer=0, random_tag=0)
    assert m.heads_backend == "auto"
    m._heads = {("cpu", 0, b): b for b in ("auto", "large", "broad")}      # (what heads() would have built: only the key is looked up)
    m._heads_version = {k: m.weights_version() for k in m._heads}
    assert m.heads("cpu") == "auto" and m.heads("cpu", backend="large") == "large" and m.heads("cpu", backend="broad") == "broad"
    import muzero_cli
    block = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
                 num_simulations=5, maxium_action_sample=2, number_of_player=1, custom_loop=None)
    with_key = dict(monte_carlo_tree_search=dict(block, broad_heads=True))
    assert "broad_heads" not in muzero_cli.mcts_kwargs(with_key)
    _pkg("mcts").BatchedMCTS(4, **muzero_cli.mcts_kwargs(with_key))
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block))) is m and m.heads_backend == "auto"
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block, broad_heads=False))).heads_backend == "auto"
    with pytest.raises(ValueError):
        muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block, broad_heads=True, large_action_heads=True)))
    assert m.heads_backend == "auto"
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block, large_action_heads=True))).heads_backend == "large"
    assert muzero_cli.set_heads_backend(m, with_key).heads_backend == "broad"
    assert m.heads("cpu") == "broad" and model_mod.Muzero.heads_backend == "auto"
    wide = mr.fresh_net(4, 2, 16, 256, 1, seed=1)
    assert type(wide.heads("cpu")).__name__ == "FusedMlpHeads" and type(wide.heads("cpu", backend="auto")).__name__ == "FusedMlpHeads"
    with pytest.raises(ValueError):
        mr.fresh_net(4, 2, 8, 513, 0, seed=1).heads("cpu", backend="broad")


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_broad_kernel_uses_no_scratch_and_spills_no_vector_registers(tmp_path):
    """Every k_mlp_recurrent_broad* kernel: private_segment_fixed_size == 0 and no VGPR spills.  Reported, not asserted: the
    register and LDS figures (this build: 204 vector registers, 64 of them accumulators: two wavefronts per SIMD; 2432 bytes of
    static LDS, beside which the launch asks for the two activation tiles, 16 to 64 KB)."""
    out = tmp_path / "mlp_broad.s"
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), "smz_mlp_broad.hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k or "k_mlp_recurrent_broad" not in m.group(1):
            continue
        seen[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
                            for f in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                      "agpr_count", "sgpr_count", "group_segment_fixed_size")}
    assert len(seen) >= 1, sorted(seen)
    for n, f in sorted(seen.items()):
        print(n, f)
    assert not {n: f["private_segment_fixed_size"] for n, f in seen.items() if f["private_segment_fixed_size"]}
    assert not {n: f["vgpr_spill_count"] for n, f in seen.items() if f["vgpr_spill_count"]}
