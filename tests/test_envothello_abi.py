"""smz_othello_reset / smz_othello_step_ctl / smz_othello_host_step / smz_othello_host_moves: declared alike by the header, the
library and the ctypes binding, in smz_connect4_step_ctl's argument order with `mover_dev` after `discs_dev`; the unit has
exactly the step kernel and the reset kernel, both keep their state in registers (no scratch memory, no spills), and the step
kernel stages the rows of kEnvs envs in LDS (the code object's resource metadata; no disassembly is read)."""
import os
import re

import pytest

from test_envconnect4_abi import CSRC, HIPCC, ROOT, _binding, kernel_resources

ENTRY_POINTS = ("smz_othello_reset", "smz_othello_step_ctl", "smz_othello_host_step", "smz_othello_host_moves")
K_ENVS = 16                                                  # GameOthello::kEnvs: the measured choice
ROW_BYTES = 263 * 8 + 65 * 4                                 # a record row (smz_traj_floats(65, 65) float64) + an observation row


def test_header_binding_and_library_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"\nint smz_othello_reset\(uint64_t \*discs_dev, int32_t \*mover_dev, float \*obs_out_dev, int B, "
                     r"smz_stream stream\);", h)
    assert re.search(r"\nint smz_othello_step_ctl\(uint64_t \*discs_dev, int32_t \*mover_dev, const int32_t \*action_dev, "
                     r"float \*obs_out_dev,\s+float \*reward_out_dev, uint8_t \*flag_out_dev, const smz_episode_ctl \*ctl, "
                     r"double \*traj_dev, int T, int t,\s+const double \*policy_dev, const double \*child_visits_dev, "
                     r"const float \*root_value_dev, int B,\s+smz_stream stream\);", h)
    assert re.search(r"\nint smz_othello_host_step\(uint64_t discs\[2\], int \*mover, int action, float \*reward_out, "
                     r"int \*terminated_out, int \*illegal_out\);", h)
    assert re.search(r"\nint smz_othello_host_moves\(const uint64_t discs\[2\], int colour, uint64_t \*mask_out\);", h)
    lib = _binding()
    step, step_c4 = lib.SIGNATURES["smz_othello_step_ctl"][1], lib.SIGNATURES["smz_connect4_step_ctl"][1]
    assert step == step_c4[:1] + step_c4[:1] + step_c4[1:] and step[6]._type_ is lib.EpisodeCtl     # Connect Four's with `mover`
    assert lib.SIGNATURES["smz_othello_step_ctl"][1] == lib.SIGNATURES["smz_2048_step_ctl"][1]      # (board + spawns there)
    assert len(lib.SIGNATURES["smz_othello_reset"][1]) == 5 and len(lib.SIGNATURES["smz_othello_host_step"][1]) == 6
    assert len(lib.SIGNATURES["smz_othello_host_moves"][1]) == 3
    so = os.path.join(ROOT, "stochastic-muzero_amd", "libsmz.so")
    if not os.path.exists(so):
        pytest.fail("libsmz.so is not built (python __graft_entry__.py build)")
    import ctypes
    built = ctypes.CDLL(so)
    for name in ENTRY_POINTS:
        assert hasattr(built, name), name


def test_the_sources_and_the_python_env_state_the_same_envs_per_workgroup():
    with open(os.path.join(CSRC, "smz_envothello.hip")) as f:
        src = f.read()
    assert int(re.search(r"#define SMZ_OTHELLO_ENVS (\d+)", src).group(1)) == K_ENVS
    with open(os.path.join(ROOT, "stochastic-muzero_amd", "envs.py")) as f:
        py = f.read()
    assert int(re.search(r"class OthelloVec.*?\n    envs_per_group = (\d+)", py, re.S).group(1)) == K_ENVS


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_the_unit_has_two_kernels_without_scratch_and_the_stated_lds(tmp_path):
    """k_board_step_env<GameOthello> and k_othello_reset are the unit's only kernels: no private segment (the position is two
    64-bit registers and the mover; every shift count and every index is a compile-time constant), no spills, and
    kEnvs x (263 float64 of record + 65 float32 of observation) bytes of LDS.  Reported, not asserted: the register counts."""
    step, reset = kernel_resources(tmp_path, "smz_envothello.hip", "GameOthello", "k_othello_reset")
    assert step["group_segment_fixed_size"] == K_ENVS * ROW_BYTES == K_ENVS * 2364
    assert reset["group_segment_fixed_size"] == 0
