"""smz_mlp_layout_broad_bf16 / smz_mlp_recurrent_broad_bf16 (csrc/smz_mlp_broad_bf16.hip): declared alike by the header, the
library and the ctypes binding; the host-side layout over its envelope; the packing of HipMlpBroadBf16Heads read back element by
element through the formula of include/smz.h -- every weight the torch bf16 rounding of the module's weight, biases exact;
the image evaluated in float64 through the kernel's address arithmetic with the contract's rounding points against the float64
rounded restatement (tests/mlp_bf16_reference.py); the Python layers around the opt-in backend; and the kernel's resource
metadata (no scratch memory, no spilled vector registers: the code object's metadata block, no disassembly is read).  Nothing
here needs a GPU."""
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
ENTRY_POINTS = ("smz_mlp_layout_broad_bf16", "smz_mlp_recurrent_broad_bf16")
# (obs, A, S, H, L): the shapes of tests/test_gpu_mlp_broad_bf16_heads.py
SHAPES = [(1, 1, 1, 1, 0), (3, 2, 5, 129, 1), (4, 2, 33, 32, 0), (4, 2, 65, 64, 0), (4, 3, 129, 130, 2), (4, 2, 100, 384, 0),
          (4, 129, 8, 256, 1), (4, 1000, 16, 200, 1), (5, 1024, 256, 512, 4)]
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
    for name in ("smz_mlp_layout_broad_bf16", "smz_mlp_layout_broad"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = b.SIGNATURES[name]
    return lib, b


def _pkg(name):
    sys.path.insert(0, ROOT)
    import stochastic_muzero_amd  # noqa: F401
    from importlib import import_module
    return import_module("stochastic-muzero_amd." + name)


def _r32(k):
    return (k + 31) & ~31


def _p(n):
    return (n + OP - 1) // OP


def _pieces(shape):
    """4-byte words of every matrix, and bias vectors of 128 floats per matrix, as include/smz.h documents them."""
    obs, A, S, H, L = shape
    ph, ps, pa = _p(H), _p(S), _p(A)
    wh, ws = _r32(H) * 64, _r32(S) * 64
    mid, pmid = (ph * wh, ph) if L > 0 else (0, 0)
    words = [ph * ws + A * ph * 64] * 2 + [mid] * 2 + [2 * ps * wh, ps * wh] + [ph * ws] * 2 + [mid] * 2 + \
            [(pa + ps) * wh] * 2 + [ph * _r32(obs) * 64, mid, ps * wh]
    biases = [ph, ph, pmid, pmid, 2 * ps, ps, ph, ph, pmid, pmid, pa + ps, pa + ps, ph, pmid, ps]
    return words, biases


def _weight(K, k, o):
    """include/smz.h: the bf16 element of weight (k, o) within a panel matrix of K inputs."""
    return (o // OP) * _r32(K) * OP + (k // 32) * 4096 + (o % OP // 16) * 512 + ((k % 32 // 8) * 16 + o % 16) * 8 + k % 8


def _torch_bf16_bits(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_header_and_binding_declare_the_bf16_entry_points():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"\nint smz_mlp_layout_broad_bf16\(smz_mlp_desc \*desc\);", h)
    assert re.search(r"\nint smz_mlp_recurrent_broad_bf16\(const smz_mlp_desc \*desc, const void \*weights_dev, "
                     r"const float \*parent_hidden_dev,\s+const int32_t \*last_action_dev, const uint8_t \*branch_dev, "
                     r"float \*hidden_out_dev,\s+float \*reward_out_dev, float \*policy_out_dev, float \*value_out_dev, int B, "
                     r"smz_stream stream\);", h)
    for phrase in ("round-to-nearest-even", "Biases are float32", "UNROUNDED float32", "NOT torch.autocast"):
        assert phrase in h, phrase
    lib = _binding()
    assert len(lib.SIGNATURES["smz_mlp_layout_broad_bf16"][1]) == 1
    assert lib.SIGNATURES["smz_mlp_recurrent_broad_bf16"] == lib.SIGNATURES["smz_mlp_recurrent_broad"]
    for name in ENTRY_POINTS:
        assert lib.SIGNATURES[name][1][0]._type_ is lib.MlpDesc


def test_the_library_exports_the_bf16_entry_points():
    lib, _ = _host_lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_accepts_the_envelope_and_sums_to_the_documented_pieces(shape):
    lib, b = _host_lib()
    d = b.MlpDesc(*shape)
    assert lib.smz_mlp_layout_broad_bf16(C.byref(d)) == 0 and d.OP == OP
    words, biases = _pieces(shape)
    off = 0
    for m in range(15):
        assert d.off[m] == off and off % 4 == 0, m            # (words: 16-byte aligned)
        off += words[m]
    for m in range(15):
        assert d.off[15 + m] == off and off % 4 == 0, m
        off += biases[m] * OP
    assert d.total_floats == off
    _, A, S, H, _ = shape
    for m in (M_DYN_IN, M_ADY_IN):                            # the action table behind the hidden part's panels
        assert d.off[m] + _p(H) * (_r32(S) + A) * 64 == d.off[m + 1]
    assert d.off[M_ADY_IN] + _p(H) * (_r32(S) + A + 1) * 64 <= d.total_floats      # a table is never the image's last piece
    f32 = b.MlpDesc(*shape)                                   # never the float32 layout's descriptor
    assert lib.smz_mlp_layout_broad(C.byref(f32)) == 0 and list(f32.off) != list(d.off)


def test_layout_refuses_what_is_outside_the_envelope():
    lib, b = _host_lib()
    for shape in [(4, 2, 8, 513, 0), (4, 2, 257, 64, 0), (4, 1025, 8, 16, 0)]:
        assert lib.smz_mlp_layout_broad_bf16(C.byref(b.MlpDesc(*shape))) == b.SMZ_ERR_TOO_LARGE, shape
    for shape in [(4, 0, 8, 16, 0), (0, 2, 8, 16, 0), (4, 2, 0, 16, 0), (4, 2, 8, 0, 0), (4, 2, 8, 16, -1), (4, -1, 8, 16, 0),
                  (4, 2, -8, 16, 0), (4, 2, 8, -16, 0), (-4, 2, 8, 16, 0)]:
        assert lib.smz_mlp_layout_broad_bf16(C.byref(b.MlpDesc(*shape))) == b.SMZ_ERR_INVALID, shape
    assert lib.smz_mlp_layout_broad_bf16(None) == b.SMZ_ERR_INVALID
    for shape in [(4, 2, 8, 512, 0), (4, 2, 256, 64, 0), (4, 1024, 8, 16, 0)]:      # (the limits themselves)
        assert lib.smz_mlp_layout_broad_bf16(C.byref(b.MlpDesc(*shape))) == 0, shape


def _fresh(shape, seed):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mlp_reference as mr
    model_mod = _pkg("model")
    model = mr.fresh_net(*shape, seed=seed, gain=4)
    w = {k: np.asarray(v) for k, v in model_mod.mlp_arrays_from_modules(
        model.representation_function, model.prediction_function, model.afterstate_prediction_function,
        model.afterstate_dynamics_function, model.dynamics_function).items()}
    return model, w


def _packed(shape, w):
    heads_mod, lib_mod = _pkg("heads"), _pkg("_lib")
    d = lib_mod.MlpDesc(*shape)
    assert lib_mod.load().smz_mlp_layout_broad_bf16(C.byref(d)) == 0
    img = heads_mod.HipMlpBroadBf16Heads.pack(w, d)
    assert img.dtype == np.uint32 and img.size == d.total_floats and sys.byteorder == "little"
    return d, img


def test_the_packers_rounding_is_torchs():
    """HipMlpBroadBf16Heads.round_bf16 on ties (to even, both ways), values next to ties, subnormals, infinities, the largest
    finite float (rounds to infinity) and 100 000 random bit patterns: torch's float32 -> bfloat16 cast, bit for bit."""
    heads_mod = _pkg("heads")
    rng = np.random.default_rng(3)
    bits = np.concatenate([np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x00008000, 0x00018000,
                                     0x00000001, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0, 0x80000000], np.uint32),
                           rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)])
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]
    assert np.array_equal(heads_mod.HipMlpBroadBf16Heads.round_bf16(x), _torch_bf16_bits(x))


def test_packing_round_trip():
    """The packed image of a fresh (4,129,130,131,2) net read back with the formula of include/smz.h: every weight of every
    matrix (hidden parts, action-table rows, the reward / state and policy / value column ranges in panels of their own) is the
    torch bf16 rounding of the module's weight, every bias is exact; no element claimed twice; everything else in the image
    exactly 0."""
    shape = (4, 129, 130, 131, 2)
    obs, A, S, H, L = shape
    _, w = _fresh(shape, 5)
    d, img = _packed(shape, w)
    halves, floats = img.view(np.uint16), img.view(np.float32)
    seen = np.zeros(halves.size, bool)                        # per bf16 element; a bias word claims both of its halves

    def claim(idx, what):
        idx = np.asarray(idx).reshape(-1)
        assert not seen[idx].any() and np.unique(idx).size == idx.size, what
        seen[idx] = True

    def matrix(base, bias, W, b, what):
        """W [O, K] (torch layout), b [O]: a panel matrix at word base, its biases at word bias."""
        O, K = W.shape
        k, o = np.meshgrid(np.arange(K), np.arange(O), indexing="ij")
        idx = (2 * base + _weight(K, k, o)).reshape(-1)
        claim(idx, what)
        assert np.array_equal(halves[idx], _torch_bf16_bits(W.T.reshape(-1))), what
        words = bias + np.arange(O)
        claim(np.concatenate([2 * words, 2 * words + 1]), what + " bias")
        assert np.array_equal(floats[words].view(np.uint32), np.asarray(b, np.float32).view(np.uint32)), what + " bias"
        return base + _p(O) * _r32(K) * 64, bias + _p(O) * OP

    for tag, m in (("dyn", M_DYN_IN), ("ady", M_ADY_IN)):
        W, b = w[tag + "_in_w"], w[tag + "_in_b"]             # [H, S + A]
        table, _ = matrix(d.off[m], d.off[15 + m], W[:, :S], b, tag + "_in")
        assert table == d.off[m] + _p(H) * _r32(S) * 64
        a, o = np.meshgrid(np.arange(A), np.arange(H), indexing="ij")      # (rows 0, 127, 128 among them)
        idx = (2 * table + a * OP * _p(H) + o).reshape(-1)
        claim(idx, tag + " table")
        assert np.array_equal(halves[idx], _torch_bf16_bits(W[:, S:].T.reshape(-1))), tag + " table"
    at, bias = matrix(d.off[M_DYN_OUT], d.off[15 + M_DYN_OUT], w["dyn_rw_w"], w["dyn_rw_b"], "reward")
    assert (at, bias) == (d.off[M_DYN_OUT] + _p(S) * _r32(H) * 64, d.off[15 + M_DYN_OUT] + _p(S) * OP)
    matrix(at, bias, w["dyn_st_w"], w["dyn_st_b"], "state")
    for tag, m in (("pre", M_PRE_OUT), ("apr", M_APR_OUT)):
        at, bias = matrix(d.off[m], d.off[15 + m], w[tag + "_pol_w"], w[tag + "_pol_b"], tag + " policy")
        assert (at, bias) == (d.off[m] + _p(A) * _r32(H) * 64, d.off[15 + m] + _p(A) * OP)
        matrix(at, bias, w[tag + "_val_w"], w[tag + "_val_b"], tag + " value")
    for m, name in ((M_DYN_MID, "dyn_mid"), (M_ADY_MID, "ady_mid"), (M_ADY_OUT, "ady_st"), (M_PRE_IN, "pre_in"), (M_APR_IN, "apr_in"),
                    (M_PRE_MID, "pre_mid"), (M_APR_MID, "apr_mid"), (M_REP_IN, "rep_in"), (M_REP_MID, "rep_mid"), (M_REP_OUT, "rep_out")):
        matrix(d.off[m], d.off[15 + m], w[name + "_w"], w[name + "_b"], name)
    assert 0 < seen.sum() < halves.size and (halves[~seen] == 0).all()
    n_weights = sum(v.size for k, v in w.items() if k.endswith("_w"))
    n_biases = sum(v.size for k, v in w.items() if k.endswith("_b"))
    assert seen.sum() == n_weights + 2 * n_biases


def test_the_image_read_with_the_kernels_addresses_gives_the_rounded_restatements_outputs():
    """The packed image of a fresh (4,129,130,131,2) net evaluated in float64 numpy through the address arithmetic of
    csrc/smz_mlp_broad_bf16_device.hpp -- 32-input steps of 8 tiles of 64 fragments, 128-column panels with a float32 bias
    vector each, hidden part + bf16 action-table row, reward / state and policy / value panels -- with every layer input rounded
    to bf16 where the kernel writes it into its LDS tile, on 64 rows of mixed branches with actions 0, 127, 128 and A - 1 among
    them: the float64 rounded restatement's hidden rows, policies and logits to 1e-6 (both sides float64 with the same roundings)."""
    import torch
    shape = (4, 129, 130, 131, 2)
    obs, A, S, H, L = shape
    model, w = _fresh(shape, 6)
    import mlp_bf16_reference as br16
    d, img = _packed(shape, w)
    with np.errstate(invalid="ignore"):                       # (the halves of a float32 bias word are no bf16 values)
        halves = (img.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)  # every half as a bf16 value
    floats = img.view(np.float32).astype(np.float64)                                                # every word as a float32 value
    rnd = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16).double().numpy()   # the tile store

    def panel(base, bias, x, K32):
        """bf16_layer: x [32 K32] -> 128 outputs, fragment of lane l of tile t in step s at bf16 element ((s * 8 + t) * 64 + l) * 8"""
        out = floats[bias + np.arange(OP)].copy()
        k = np.arange(32 * K32)
        for o in range(OP):
            lane = (k % 32 // 8) * 16 + o % 16
            out[o] += (x * halves[2 * base + (((k // 32) * 8 + o // 16) * 64 + lane) * 8 + k % 8]).sum()
        return out

    def layer(base, bias, x, K32, panels, first=0):
        """panels first .. first + panels - 1 of the matrix at word base, one after the other"""
        return np.concatenate([panel(base + p * K32 * 2048, bias + p * OP, x, K32) for p in range(first, first + panels)])

    elu = lambda v: np.where(v > 0, v, np.exp(np.minimum(v, 0)) - 1)
    pad = lambda v, n: np.concatenate([v, np.zeros(n - v.size)])
    g = torch.Generator().manual_seed(9)
    rows = 64
    h = torch.rand(rows, S, generator=g)
    a = torch.randint(0, A, (rows,), generator=g)
    a[:4] = torch.tensor([0, 127, 128, A - 1])
    br = torch.randint(0, 2, (rows,), generator=g)
    assert 0 < int(br.sum()) < rows
    r64 = br16.RoundedRestatement(model)
    recurrent = [getattr(model, f + "_function") for f in ("prediction", "afterstate_prediction", "afterstate_dynamics", "dynamics")]
    assert r64.linears == len({id(x) for f in recurrent for x in f.modules() if isinstance(x, torch.nn.Linear)}) >= 4 * 3
    want = r64.recurrent(h, a, br)
    K32s, K32h, PH, PS, PA = _r32(S) // 32, _r32(H) // 32, _p(H), _p(S), _p(A)
    for i in range(rows):
        ady = int(br[i]) == 0
        off = lambda m: (d.off[m + (1 if ady else 0)], d.off[15 + m + (1 if ady else 0)])
        (w_in, b_in), (w_mid, b_mid), (w_out, b_out) = off(M_DYN_IN), off(M_DYN_MID), off(M_DYN_OUT)
        (p_in, pb_in), (p_mid, pb_mid), (p_out, pb_out) = off(M_PRE_IN), off(M_PRE_MID), off(M_PRE_OUT)
        y = layer(w_in, b_in, pad(rnd(h[i].double().numpy()), 32 * K32s), K32s, PH)
        table = 2 * (w_in + PH * K32s * 2048) + int(a[i]) * PH * OP
        y = y + halves[table:table + PH * OP]
        assert (y[H:] == 0).all()                             # (padding columns: the padding inputs of the next layer)
        t = rnd(elu(y))[:32 * K32h]
        for _ in range(L):
            t = rnd(elu(layer(w_mid, b_mid, t, K32h, PH)))[:32 * K32h]
        if ady:
            state = layer(w_out, b_out, t, K32h, PS)[:S]
        else:
            np.testing.assert_allclose(layer(w_out, b_out, t, K32h, PS)[:S], want["reward_logits"][i].numpy(), rtol=0, atol=1e-6)
            state = layer(w_out, b_out, t, K32h, PS, first=PS)[:S]
        span = state.max() - state.min()
        hid = (state - state.min()) / (span + 1e-5 if span < 1e-5 else span)
        np.testing.assert_allclose(hid, want["hidden"][i].numpy(), rtol=0, atol=1e-6)       # (hidden_out: unrounded)
        t = rnd(elu(layer(p_in, pb_in, pad(rnd(hid), 32 * K32s), K32s, PH)))[:32 * K32h]
        for _ in range(L):
            t = rnd(elu(layer(p_mid, pb_mid, t, K32h, PH)))[:32 * K32h]
        logits = layer(p_out, pb_out, t, K32h, PA)[:A]
        e = np.exp(logits - logits.max())
        np.testing.assert_allclose(e / e.sum(), want["policy"][i].numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(layer(p_out, pb_out, t, K32h, PS, first=PA)[:S], want["value_logits"][i].numpy(), rtol=0, atol=1e-6)


def test_python_layers_around_the_backend():
    """Muzero.heads_backend stays "auto"; the CLI sets "broad_bf16" from the config key "broad_bf16_heads" and keeps the key away
    from BatchedMCTS; the key together with "large_action_heads" or "broad_heads" raises; "auto" and "broad" keep looking up what
    they looked up; heads(backend="broad_bf16") raises ValueError outside the limits."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mlp_reference as mr
    model_mod, heads_mod = _pkg("model"), _pkg("heads")
    assert model_mod.Muzero.heads_backend == "auto"
    cls = heads_mod.HipMlpBroadBf16Heads
    assert issubclass(cls, heads_mod.FusedMlpHeads) and not issubclass(cls, heads_mod.HipMlpBroadHeads)
    assert (cls.wants_mlp_input, cls.wants_parent_hidden) == (False, True)
    assert cls.single_launch is None and cls.initial is heads_mod.FusedMlpHeads.initial
    assert isinstance(cls.__dict__["pack"], staticmethod)
    m = model_mod.Muzero(model_structure="mlp_model", observation_space_dimensions=4, action_space_dimensions=40,
                         state_space_dimensions=8, hidden_layer_dimensions=16, number_of_hidden_layer=0, random_tag=0)
    assert m.heads_backend == "auto" and m.use_amp is False
    names = ("auto", "large", "broad", "broad_bf16")
    m._heads = {("cpu", 0, b): b for b in names}      # (what heads() would have built: only the key is looked up)
    m._heads_version = {k: m.weights_version() for k in m._heads}
    assert m.heads("cpu") == "auto" and all(m.heads("cpu", backend=b) == b for b in names)
    assert m.heads("cpu", backend="broad_bf16", hip_root=None) == "broad_bf16"
    import muzero_cli
    block = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
                 num_simulations=5, maxium_action_sample=2, number_of_player=1, custom_loop=None)
    with_key = dict(monte_carlo_tree_search=dict(block, broad_bf16_heads=True))
    assert "broad_bf16_heads" not in muzero_cli.mcts_kwargs(with_key)
    _pkg("mcts").BatchedMCTS(4, **muzero_cli.mcts_kwargs(with_key))
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block))) is m and m.heads_backend == "auto"
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block, broad_bf16_heads=False))).heads_backend == "auto"
    for other in ("large_action_heads", "broad_heads"):
        with pytest.raises(ValueError):
            muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block, broad_bf16_heads=True, **{other: True})))
        assert m.heads_backend == "auto"
    assert muzero_cli.set_heads_backend(m, dict(monte_carlo_tree_search=dict(block, broad_heads=True))).heads_backend == "broad"
    assert muzero_cli.set_heads_backend(m, with_key).heads_backend == "broad_bf16"
    assert m.heads("cpu") == "broad_bf16" and model_mod.Muzero.heads_backend == "auto"
    wide = mr.fresh_net(4, 2, 16, 256, 1, seed=1)
    assert type(wide.heads("cpu")).__name__ == "FusedMlpHeads" and type(wide.heads("cpu", backend="auto")).__name__ == "FusedMlpHeads"
    for shape in [(4, 2, 8, 513, 0), (4, 2, 257, 64, 0), (4, 1025, 8, 16, 0)]:
        with pytest.raises(ValueError):
            mr.fresh_net(*shape, seed=1).heads("cpu", backend="broad_bf16")


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_bf16_kernel_uses_no_scratch_and_spills_no_vector_registers(tmp_path):
    """Every k_mlp_recurrent_broad_bf16* kernel: private_segment_fixed_size == 0 and no VGPR spills.  Reported, not asserted: the
    register and LDS figures (this build: 232 vector registers, 64 of them accumulators: two wavefronts per SIMD; 2432 bytes of
    static LDS, beside which the launch asks for the two activation tiles, 2 to 32 KB)."""
    out = tmp_path / "mlp_broad_bf16.s"
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), "smz_mlp_broad_bf16.hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k or "k_mlp_recurrent_broad_bf16" not in m.group(1):
            continue
        seen[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
                            for f in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                      "agpr_count", "sgpr_count", "group_segment_fixed_size")}
    assert len(seen) == 2, sorted(seen)
    for n, f in sorted(seen.items()):
        print(n, f)
    assert not {n: f["private_segment_fixed_size"] for n, f in seen.items() if f["private_segment_fixed_size"]}
    assert not {n: f["vgpr_spill_count"] for n, f in seen.items() if f["vgpr_spill_count"]}
