"""smz_connect4_reset / smz_connect4_step_ctl / smz_connect4_host_step: declared alike by the header, the library and the ctypes
binding, in smz_2048_step_ctl's argument order without `spawns`; the step kernel keeps the position in registers (no scratch
memory, no spills) and stages a workgroup's rows in the LDS the design states (the code object's resource metadata; no
disassembly is read)."""
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
ENTRY_POINTS = ("smz_connect4_reset", "smz_connect4_step_ctl", "smz_connect4_host_step")
FIELDS = ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "sgpr_count")


def _binding():
    import importlib.util
    spec = importlib.util.spec_from_file_location("smz_lib_only", os.path.join(ROOT, "stochastic-muzero_amd", "_lib.py"))
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    return lib


def kernel_resources(tmp_path, source, game, reset_name):
    """-> the resource metadata of (k_board_step_env<game>, the reset kernel), the unit's only two kernels, both without scratch
    memory and spills."""
    out = tmp_path / (source + ".s")
    p = subprocess.run([HIPCC, *FLAGS, "-o", str(out), source], cwd=CSRC, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k:
            continue
        seen[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1)) for f in FIELDS}
    for n, f in sorted(seen.items()):
        print(n, f)
    step = [f for n, f in seen.items() if "k_board_step_env" in n and game in n]
    reset = [f for n, f in seen.items() if reset_name in n]
    assert len(step) == 1 and len(reset) == 1 and len(seen) == 2, sorted(seen)
    for f in step + reset:
        assert (f["private_segment_fixed_size"], f["vgpr_spill_count"], f["sgpr_spill_count"]) == (0, 0, 0), f
    return step[0], reset[0]


def test_header_binding_and_library_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"\nint smz_connect4_reset\(uint64_t \*discs_dev, float \*obs_out_dev, int B, smz_stream stream\);", h)
    assert re.search(r"\nint smz_connect4_step_ctl\(uint64_t \*discs_dev, const int32_t \*action_dev, float \*obs_out_dev, "
                     r"float \*reward_out_dev,\s+uint8_t \*flag_out_dev, const smz_episode_ctl \*ctl, double \*traj_dev, int T, int t,"
                     r"\s+const double \*policy_dev, const double \*child_visits_dev, const float \*root_value_dev, int B,"
                     r"\s+smz_stream stream\);", h)
    assert re.search(r"\nint smz_connect4_host_step\(uint64_t discs\[2\], int action, float \*reward_out, int \*terminated_out, "
                     r"int \*illegal_out\);", h)
    lib = _binding()
    step, step2048 = lib.SIGNATURES["smz_connect4_step_ctl"][1], lib.SIGNATURES["smz_2048_step_ctl"][1]
    assert step == step2048[:1] + step2048[2:] and step[5]._type_ is lib.EpisodeCtl          # 2048's order without `spawns`
    assert len(lib.SIGNATURES["smz_connect4_reset"][1]) == 4 and len(lib.SIGNATURES["smz_connect4_host_step"][1]) == 5
    so = os.path.join(ROOT, "stochastic-muzero_amd", "libsmz.so")
    if not os.path.exists(so):
        pytest.fail("libsmz.so is not built (python __graft_entry__.py build)")
    import ctypes
    built = ctypes.CDLL(so)
    for name in ENTRY_POINTS:
        assert hasattr(built, name), name


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_the_step_kernel_has_no_scratch_and_the_stated_lds(tmp_path):
    """k_board_step_env<GameConnect4>: no private segment (the position is two 64-bit registers and no array is indexed with a
    run-time value), no spills, and 64 x 67 float64 record rows + 64 x 43 float32 observation rows of LDS = 45 312 bytes.
    Reported, not asserted: the register counts."""
    step, reset = kernel_resources(tmp_path, "smz_envconnect4.hip", "GameConnect4", "k_connect4_reset")
    assert step["group_segment_fixed_size"] == 64 * 67 * 8 + 64 * 43 * 4 == 45312
    assert reset["group_segment_fixed_size"] == 0
