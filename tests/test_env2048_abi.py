"""The 2048 step kernel, k_board_step_env<Game2048> (csrc/smz_env_frame.hpp): the kernel Connect Four's env runs, over the other
game (the code object's resource metadata; no disassembly is read)."""
import os

import pytest

from test_envconnect4_abi import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_the_step_kernel_has_no_scratch_and_the_stated_lds(tmp_path):
    """No private segment (the board is four 32-bit registers), no spills, and 64 x 31 float64 record rows of LDS = 15 872
    bytes: the observation rows are not staged (Game2048::kStageObs = false)."""
    step, reset = kernel_resources(tmp_path, "smz_env2048.hip", "Game2048", "k_2048_reset")
    assert step["group_segment_fixed_size"] == 64 * 31 * 8 == 15872
    assert reset["group_segment_fixed_size"] == 0
