"""smz_mlp_initial_broad (csrc/smz_mlp_broad_root.hip): declared alike by the header, the library and the ctypes binding; the
refusals the launcher makes on the host before any HIP call; the Python layers around the opt-in `hip_root` of the two broad head
classes, on "cpu" heads (the constructors launch nothing); and the kernel's resource metadata (no scratch memory, no spilled
vector registers: the code object's metadata block, no disassembly is read).  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_mlp_large_abi import CSRC, FLAGS, HIPCC, ROOT, M_REP_OUT, _binding, _pkg

ENTRY = "smz_mlp_initial_broad"
SHAPE = (9, 129, 5, 7, 2)
# the four other layouts, each on a shape it accepts
OTHERS = (("smz_mlp_layout", (9, 3, 5, 7, 2)), ("smz_mlp_layout_wide", (9, 3, 5, 7, 2)), ("smz_mlp_layout_large", SHAPE),
          ("smz_mlp_layout_broad_bf16", SHAPE))
BACKENDS = (("broad", "HipMlpBroadHeads"), ("broad_bf16", "HipMlpBroadBf16Heads"))


def _host_lib():
    so = os.path.join(ROOT, "stochastic-muzero_amd", "libsmz.so")
    if not os.path.exists(so):
        pytest.fail("libsmz.so is not built (python __graft_entry__.py build)")
    lib = C.CDLL(so)
    b = _binding()
    for name in (ENTRY, "smz_mlp_layout_broad") + tuple(n for n, _ in OTHERS):
        assert hasattr(lib, name), name
        getattr(lib, name).restype, getattr(lib, name).argtypes = b.SIGNATURES[name]
    return lib, b


def test_header_binding_and_library_declare_the_entry_point():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"\nint %s\s*\(const smz_mlp_desc \*desc, const float \*weights_dev, const float \*obs_dev,\s+"
                     r"float \*hidden_out_dev,\s+float \*policy_out_dev, int B, smz_stream stream\);" % ENTRY, h)
    b = _binding()
    res, args = b.SIGNATURES[ENTRY]
    assert res is C.c_int and len(args) == 7 and args[0]._type_ is b.MlpDesc and args[5] is C.c_int
    assert args == b.SIGNATURES["smz_mlp_initial"][1]
    lib, _ = _host_lib()
    assert hasattr(lib, ENTRY)


def test_the_launcher_refuses_on_the_host_before_any_hip_call():
    """Null pointers and B < 1 -> SMZ_ERR_INVALID; a descriptor of smz_mlp_layout, _wide, _large or _broad_bf16 -> SMZ_ERR_INVALID;
    a broad descriptor with a changed total or offset -> SMZ_ERR_INVALID; obs = 1025 -> SMZ_ERR_TOO_LARGE, and obs = 1025 with a
    null pointer still SMZ_ERR_INVALID.  The device pointers are dummies: every one of these calls returns before it would
    touch them (no GPU on this side of the suite)."""
    lib, b = _host_lib()
    fn = getattr(lib, ENTRY)
    d = b.MlpDesc(*SHAPE)
    assert lib.smz_mlp_layout_broad(C.byref(d)) == 0
    dummy = C.c_void_p(4096)
    args = [C.byref(d), dummy, dummy, dummy, dummy, 8, None]
    for i in range(5):
        assert fn(*[None if j == i else x for j, x in enumerate(args)]) == b.SMZ_ERR_INVALID, i
    assert fn(*args[:5], 0, None) == b.SMZ_ERR_INVALID and fn(*args[:5], -3, None) == b.SMZ_ERR_INVALID
    for layout, shape in OTHERS:
        other = b.MlpDesc(*shape)
        assert getattr(lib, layout)(C.byref(other)) == 0, layout
        assert fn(C.byref(other), *args[1:]) == b.SMZ_ERR_INVALID, layout
    # the shape of the broad descriptor itself in the layouts that take it: other images, refused
    for layout in ("smz_mlp_layout_large", "smz_mlp_layout_broad_bf16"):
        other = b.MlpDesc(*SHAPE)
        assert getattr(lib, layout)(C.byref(other)) == 0 and other.total_floats != d.total_floats
    bad = b.MlpDesc.from_buffer_copy(d)
    bad.total_floats += 128
    assert fn(C.byref(bad), *args[1:]) == b.SMZ_ERR_INVALID
    bad = b.MlpDesc.from_buffer_copy(d)
    bad.off[M_REP_OUT] += 128
    assert fn(C.byref(bad), *args[1:]) == b.SMZ_ERR_INVALID
    bad = b.MlpDesc(*SHAPE)                                  # (never laid out: OP = 0)
    assert fn(C.byref(bad), *args[1:]) == b.SMZ_ERR_INVALID
    wide_obs = b.MlpDesc(1025, *SHAPE[1:])
    assert lib.smz_mlp_layout_broad(C.byref(wide_obs)) == 0
    assert fn(C.byref(wide_obs), *args[1:]) == b.SMZ_ERR_TOO_LARGE
    assert fn(C.byref(wide_obs), None, *args[2:]) == b.SMZ_ERR_INVALID and fn(C.byref(wide_obs), *args[1:5], 0, None) == b.SMZ_ERR_INVALID


def _arrays(model):
    model_mod = _pkg("model")
    return {k: np.asarray(v) for k, v in model_mod.mlp_arrays_from_modules(
        model.representation_function, model.prediction_function, model.afterstate_prediction_function,
        model.afterstate_dynamics_function, model.dynamics_function).items()}


def test_python_layers_around_hip_root_on_the_broad_heads():
    """Both classes take hip_root (default False) and keep FusedMlpHeads.initial as their class attribute.  Without the flag an
    instance has no `initial` of its own and the bf16 heads no root_packed; with it both have an instance `initial`, and the bf16
    heads' root_packed is HipMlpBroadHeads.pack of the same arrays on a smz_mlp_layout_broad descriptor, element for element.
    obs = 1025 with hip_root=True raises HipRootLimit (a ValueError naming the limit) for both backends and builds without the
    flag.  Muzero.heads(backend=..., hip_root=True) caches under a key of its own, passes the flag on, and heads(hip_root=None)
    follows model.hip_root."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mlp_reference as mr
    model_mod, heads_mod, lib_mod = _pkg("model"), _pkg("heads"), _pkg("_lib")
    shape = (9, 129, 130, 131, 1)
    dims = dict(zip(("obs", "A", "S", "H", "L"), shape))
    model = mr.fresh_net(*shape, seed=3, gain=4)
    w = _arrays(model)
    for backend, name in BACKENDS:
        cls = getattr(heads_mod, name)
        assert inspect.signature(cls.__init__).parameters["hip_root"].default is False
        assert cls.initial is heads_mod.FusedMlpHeads.initial and cls.single_launch is None
        plain = cls(w, dims, "cpu")
        assert plain.hip_root is False and "initial" not in vars(plain) and "root_packed" not in vars(plain) and "root_desc" not in vars(plain)
        assert plain.initial.__func__ is heads_mod.FusedMlpHeads.initial
        flagged = cls(w, dims, "cpu", hip_root=True)
        assert flagged.hip_root is True and "initial" in vars(flagged) and callable(flagged.initial)
        assert flagged.packed.dtype == plain.packed.dtype and np.array_equal(flagged.packed.numpy(), plain.packed.numpy())
        if backend == "broad_bf16":
            d = lib_mod.MlpDesc(*shape)
            assert lib_mod.load().smz_mlp_layout_broad(C.byref(d)) == 0
            want = heads_mod.HipMlpBroadHeads.pack(w, d)
            got = flagged.root_packed.numpy()
            assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            assert flagged.root_desc.total_floats == d.total_floats and list(flagged.root_desc.off) == list(d.off)
            assert flagged.root_desc.total_floats != flagged.broad_bf16_desc.total_floats
            f32 = heads_mod.HipMlpBroadHeads(w, dims, "cpu", hip_root=True)
            assert np.array_equal(f32.packed.numpy().view(np.uint32), got.view(np.uint32))
        else:
            assert "root_packed" not in vars(flagged)
        # through Muzero.heads: a key of its own, the flag passed on
        a = model.heads("cpu", backend=backend)
        b2 = model.heads("cpu", backend=backend, hip_root=True)
        assert type(a).__name__ == name and type(b2).__name__ == name and a is not b2
        assert not a.hip_root and "initial" not in vars(a) and b2.hip_root and "initial" in vars(b2)
        assert model.heads("cpu", backend=backend, hip_root=False) is a and model.heads("cpu", backend=backend, hip_root=True) is b2
        assert ("cpu", 0, backend) in model._heads and ("cpu", 0, backend, "hip_root") in model._heads
        model.hip_root = True
        assert model.heads("cpu", backend=backend) is b2
        model.hip_root = False
        assert model.heads("cpu", backend=backend) is a
    assert model_mod.Muzero.hip_root is False
    heads_mod._check_hip_root(lib_mod.load(), 1024, ENTRY)
    wide = mr.fresh_net(1025, 3, 8, 16, 0, seed=1)
    for backend, name in BACKENDS:
        assert type(wide.heads("cpu", backend=backend)).__name__ == name
        with pytest.raises(heads_mod.HipRootLimit, match="1024"):
            wide.heads("cpu", backend=backend, hip_root=True)
        assert ("cpu", 0, backend, "hip_root") not in wide._heads


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_broad_root_kernel_uses_no_scratch_and_spills_no_vector_registers(tmp_path):
    """Every k_mlp_initial_broad* kernel of smz_mlp_broad_root.hip: private_segment_fixed_size == 0 and no VGPR spills.  Reported,
    not asserted: the register and LDS figures (this build: 224 vector registers, 64 of them accumulators: two wavefronts per SIMD;
    1280 bytes of static LDS, beside which the launch asks for the two activation tiles, 16 to 96 KB)."""
    out = tmp_path / "mlp_broad_root.s"
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), "smz_mlp_broad_root.hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k or "k_mlp_initial_broad" not in m.group(1):
            continue
        seen[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
                            for f in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                      "agpr_count", "sgpr_count", "group_segment_fixed_size")}
    assert len(seen) >= 1, sorted(seen)
    for n, f in sorted(seen.items()):
        print(n, f)
    assert not {n: f["private_segment_fixed_size"] for n, f in seen.items() if f["private_segment_fixed_size"]}
    assert not {n: f["vgpr_spill_count"] for n, f in seen.items() if f["vgpr_spill_count"]}
