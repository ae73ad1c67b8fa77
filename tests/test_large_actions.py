"""Build-time checks of the large-action kernels (smz_large_actions.hip; no GPU: hipcc cross-compiles gfx950 here), and the
host side of smz_create_large_actions that needs no device."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stochastic-muzero_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the library's own flags (csrc/Makefile)
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-function", "-Wno-unused-variable",
         "-Wno-unused-const-variable", "-S", "--cuda-device-only"]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("make") is None or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_large_action_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """Every _la kernel keeps its A-wide arrays in LDS: no private segment, no VGPR or SGPR spills."""
    out = tmp_path / "la.s"
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), "smz_large_actions.hip"], cwd=CSRC, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = re.split(r"\n  - ", meta)[1:]
    seen = {}
    for k in kernels:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k:
            continue
        name = m.group(1)
        if "_la" not in name:
            continue
        fields = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1))
                  for f in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
        seen[name] = fields
    names = " ".join(seen)
    for kern in ("k_root_init_la", "k_root_noise_la", "k_select_la", "k_expand_backup_la", "k_act_la"):
        assert kern in names, f"{kern} missing from the ISA"
    bad = {n: f for n, f in seen.items() if any(f.values())}
    assert not bad, bad


def test_header_library_and_binding_declare_the_large_action_entry_point():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"#define SMZ_MAX_ACTIONS_LARGE 1024\b", h)
    assert "int smz_create_large_actions(const smz_config *cfg, smz_handle **out);" in h
    import importlib.util
    spec = importlib.util.spec_from_file_location("smz_lib_only", os.path.join(ROOT, "stochastic-muzero_amd", "_lib.py"))
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    assert lib.MAX_ACTIONS_LARGE == 1024 and lib.MAX_ACTIONS == 32
    assert "smz_create_large_actions" in lib.SIGNATURES


def _large_fixtures():
    import glob
    import numpy as np
    out = []
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "large_actions", "*.npz"))):
        z = np.load(p)
        if int(z["cfg_number_of_player"]) == 1:
            out.append("large_actions/" + os.path.basename(p)[:-4])
    return out


@pytest.mark.parametrize("name", _large_fixtures())
def test_oracle_replays_the_large_action_fixtures(name):
    """The oracle (oracle/smz_oracle.c, 1 .. 1024 actions) against every single-player large-action search of the reference's,
    33 to 1024 actions wide: the fixtures the GPU tests hold the wave-per-tree kernels to are pinned here as well, with every
    act output.  Above 128 actions this is what anchors the oracle's pairwise sums, wide `choice` rounds and Dirichlet draws
    to the reference; tests/test_gpu_large_actions_oracle.py then holds the kernels to the oracle on every tree."""
    import numpy as np
    import golden_util as gu
    import harness
    import orc
    cfg, cases = gu.cases(name)
    for case in cases:
        A, K, S, sims = gu.dims(cfg, case)
        mk = lambda: orc.Tree(orc.make_cfg(A, K, S, sims, pb_c_base=int(cfg["pb_c_base"]), pb_c_init=float(cfg["pb_c_init"]),  # noqa: E731
                                           discount=float(cfg["discount"]), alpha=float(cfg["root_dirichlet_alpha"]),
                                           frac=float(cfg["root_exploration_fraction"])))
        t = harness.drive_tape(mk(), cfg, case)
        harness.check_search_outputs(t, cfg, case)
        for T in gu.TEMPERATURES:
            t2 = harness.drive_tape(mk(), cfg, case, check_inputs=False)
            action, policy, child_visits, root_value = t2.act(T)
            k = f"T{T}"
            assert action == int(case[k + "_action"]) and root_value == case[k + "_root_value"], (T, A)
            assert np.array_equal(policy, case[k + "_policy"]) and np.array_equal(child_visits, case[k + "_child_visits"]), T
            assert t2.random_sample() == case[k + "_probe"], T


def test_oracle_refuses_more_than_1024_actions():
    """orc_tree_new sizes its stack arrays for 1 .. 1024 actions and sampled children and returns NULL outside that range."""
    import ctypes as C
    import orc
    for A, K in ((1025, 2), (0, 1), (2000, 2000)):
        with pytest.raises(ValueError):
            orc.Tree(orc.make_cfg(A, K, 3, 4))
    pbc = orc.pbc_table(19652, 1.25, 6)
    for A, K in ((4, 0), (4, 1025), (-1, 2)):                 # (make_cfg clips K to A: the library itself is asked here)
        assert not orc.lib().orc_tree_new(C.byref(orc.Cfg(A, K, 3, 4, 19652, 1.25, 0.95, 0.25, 0.25)), pbc.ctypes.data_as(C.c_void_p))
    assert orc.Tree(orc.make_cfg(1024, 1024, 3, 1)).h
