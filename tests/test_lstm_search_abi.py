"""smz_search_lstm / smz_search_lstm_act: declared alike by the header, the library and the ctypes binding; the kernel's
instantiations use no scratch memory and spill no registers (the code object's resource metadata; no disassembly is read)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stochastic-muzero_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the library's own flags (csrc/Makefile)
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-function", "-Wno-unused-variable",
         "-Wno-unused-const-variable", "-S", "--cuda-device-only"]
ENTRY_POINTS = ("smz_search_lstm", "smz_search_lstm_act")


def _binding():
    import importlib.util
    spec = importlib.util.spec_from_file_location("smz_lib_only", os.path.join(ROOT, "stochastic-muzero_amd", "_lib.py"))
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    return lib


def test_header_and_binding_declare_the_lstm_search_entry_points():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"\nint smz_search_lstm\(smz_handle \*h, const smz_lstm_desc \*desc, const float \*weights_dev, "
                     r"const float \*hidden0_dev,\s+const float \*policy0_dev, int train, smz_stream stream\);", h)
    assert re.search(r"\nint smz_search_lstm_act\(smz_handle \*h, const smz_lstm_desc \*desc, const float \*weights_dev, "
                     r"const float \*hidden0_dev,\s+const float \*policy0_dev, int train, double temperature, "
                     r"const double \*pow_table_host,\s+int32_t \*action_dev, double \*policy_dev, double \*child_visits_dev, "
                     r"float \*root_value_dev,\s+smz_stream stream\);", h)
    lib = _binding()
    assert len(lib.SIGNATURES["smz_search_lstm"][1]) == 7 and len(lib.SIGNATURES["smz_search_lstm_act"][1]) == 13
    for name in ENTRY_POINTS:
        assert lib.SIGNATURES[name][1][1]._type_ is lib.LstmDesc


def test_the_library_exports_the_lstm_search_entry_points():
    so = os.path.join(ROOT, "stochastic-muzero_amd", "libsmz.so")
    if not os.path.exists(so):
        pytest.fail("libsmz.so is not built (python __graft_entry__.py build)")
    import ctypes
    lib = ctypes.CDLL(so)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_python_layers_accept_the_flag():
    """BatchedMCTS(lstm_single_launch=...) defaults to off; SearchEngine has search_lstm; the CLI passes the config key through
    and leaves a config without it alone."""
    import inspect
    import sys
    sys.path.insert(0, ROOT)
    import stochastic_muzero_amd  # noqa: F401
    from importlib import import_module
    mcts_mod, eng_mod = import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.engine")
    assert inspect.signature(mcts_mod.BatchedMCTS.__init__).parameters["lstm_single_launch"].default is False
    assert mcts_mod.BatchedMCTS(4).lstm_single_launch is False
    assert mcts_mod.BatchedMCTS(4, lstm_single_launch=True).lstm_single_launch is True
    assert list(inspect.signature(eng_mod.SearchEngine.search_lstm).parameters)[1:] == [
        "lstm_desc", "weights", "hidden0", "policy0", "train", "act_temperature"]
    import muzero_cli
    block = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
                 num_simulations=5, maxium_action_sample=2, number_of_player=1, custom_loop=None)
    assert "lstm_single_launch" not in muzero_cli.mcts_kwargs(dict(monte_carlo_tree_search=dict(block)))
    kw = muzero_cli.mcts_kwargs(dict(monte_carlo_tree_search=dict(block, lstm_single_launch=True)))
    assert kw["lstm_single_launch"] is True and mcts_mod.BatchedMCTS(4, **kw).lstm_single_launch is True


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_lstm_search_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """Every k_search_lstm instantiation of the 2- and 4-action buckets: private_segment_fixed_size == 0, no VGPR spills, no SGPR
    spills.

    The per-lane tree code (root_init_tree's Dirichlet draws above all) takes every scalar register of a wave, so the kernel keeps
    its own wave-uniform state in vector registers (in_vgpr / unpark, smz_search_frame.hpp) and runs the root expansion without a
    branch.  With that: 212-234 vector registers of the 256 a wave may hold at two workgroups per CU, nothing
    spilled (82-126 scalar registers were, before)."""
    out = tmp_path / "lstm_search.s"
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), "smz_lstm_search.hip"], cwd=CSRC, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k or "k_search_lstm" not in m.group(1):
            continue
        seen[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
                            for f in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    for bucket in (2, 4):
        for philox in (0, 1):
            assert any("k_search_lstmILi%dELb%d" % (bucket, philox) in n for n in seen), (bucket, philox, sorted(seen))
    print({n: f for n, f in seen.items()})
    assert not {n: f["private_segment_fixed_size"] for n, f in seen.items() if f["private_segment_fixed_size"]}
    assert not {n: f["vgpr_spill_count"] for n, f in seen.items() if f["vgpr_spill_count"]}
    assert not {n: f["sgpr_spill_count"] for n, f in seen.items() if f["sgpr_spill_count"]}
