"""Multi-player searches on the host side (no GPU): the constructors accept the reference's turn cycles, Player_cycle behaves as
the reference's (mcts:38-72), the depth / sign helpers reproduce the reference's trees (tests/golden/players/*.npz, written by
tools/gen_golden_players.py from the reference itself), and the multi-player kernels are in the cross-compiled library."""
import glob
import os
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAYERS = sorted("players/" + os.path.basename(p)[:-4] for p in glob.glob(os.path.join(gu.GOLDEN, "players", "*.npz")))
SEARCHES = [n for n in PLAYERS if "selfplay" not in n]


def _mcts():
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd.mcts")


def _cycle_of(cfg):
    return int(cfg.get("number_of_player", 1)), cfg.get("custom_loop")


def test_fixtures_are_present():
    assert len(SEARCHES) >= 4 and any("selfplay" in n for n in PLAYERS)


def test_constructors_accept_multi_player_cycles():
    m = _mcts()
    for kw, n in ((dict(number_of_player=2), 2), (dict(number_of_player=3), 3), (dict(custom_loop="1>2>1>3"), 4),
                  (dict(custom_loop="1>1"), 2), (dict(number_of_player=2, custom_loop="5>6>7"), 3)):
        s = m.Monte_carlo_tree_search(**kw)
        assert s.n_cycle == n and len(s.cycle.cycle_map) == n
        b = m.BatchedMCTS(16, **kw)
        assert b.n_cycle == n and b.engine is None
    assert m.Monte_carlo_tree_search(number_of_player=1).n_cycle == 1
    for bad in (dict(number_of_player=0), dict(custom_loop=3), dict(number_of_player=2.0)):
        with pytest.raises(AssertionError):
            m.Monte_carlo_tree_search(**bad)
        with pytest.raises(AssertionError):
            m.BatchedMCTS(4, **bad)
    with pytest.raises(ValueError):
        m.BatchedMCTS(4, number_of_player=33)


def test_player_cycle_traces_the_references():
    """global_step / global_reset / proximate_player_step / player_in_play as mcts:38-72 produce them."""
    m = _mcts()
    c = m.Player_cycle(number_of_player=3)
    assert [c.global_step() for _ in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    c.global_reset()
    assert c.global_step() == 0 and c.global_count == 1
    assert [c.proximate_player_step(i) for i in range(3)] == [1, 2, 0]
    assert [c.player_in_play(i) for i in range(4)] == [0, 1, 2, 0]
    c = m.Player_cycle(number_of_player=2, custom_loop="1>2>1>3")    # a string loop wins over the count (mcts:43-46)
    assert c.cycle_map == [1.0, 2.0, 1.0, 3.0]
    assert [c.global_step() for _ in range(5)] == [0, 1, 2, 3, 0]
    assert [c.player_in_play(i) for i in range(5)] == [1.0, 2.0, 1.0, 3.0, 1.0]
    with pytest.raises(Exception):
        m.Player_cycle()


def test_sign_masks():
    m = _mcts()
    assert list(m.player_sign_masks([0, 1])) == [0b10, 0b10]
    assert list(m.player_sign_masks([0, 1, 2])) == [0b110] * 3
    # "1>2>1>3": root 0 (value 1) sees 2 and 3 as the others; root 1 (value 2) sees every other entry as another player
    assert list(m.player_sign_masks([1, 2, 1, 3])) == [0b1010, 0b1110, 0b1010, 0b1110]
    assert list(m.player_sign_masks([1, 1])) == [0, 0]
    assert list(m.player_sign_masks([1, 1, 2])) == [0b100, 0b010, 0b110]


def _tree_depths(case, K):
    cb = case["tree_child_base"]
    A = int(case["root_policy"].shape[-1])
    depth = np.zeros(cb.size, np.int64)
    for i in range(cb.size):                             # parents precede their children in creation order
        if cb[i]:
            cnt = A if i == 0 else K
            depth[cb[i]:cb[i] + cnt] = depth[i] + 1
    return depth


@pytest.mark.parametrize("name", SEARCHES)
def test_to_play_by_depth_reproduces_the_references_nodes(name):
    m = _mcts()
    cfg, cases = gu.cases(name)
    L = len(m.cycle_values(*_cycle_of(cfg)))
    assert L > 1
    for c in cases:
        A, K, _, _ = gu.dims(cfg, c)
        depth = _tree_depths(c, K)
        assert np.array_equal(m.to_play_at_depth(int(c["root_to_play"]), depth, L), c["tree_to_play"])


@pytest.mark.parametrize("name", SEARCHES)
def test_signed_backup_reproduces_every_value_sum(name):
    """Replaying the recorded paths with the sign masks gives the reference's value_sum at every node -- and the single-player
    backup does not on most cases (a shallow tree whose only other player sits deeper than its paths reach cannot tell)."""
    m = _mcts()
    cfg, cases = gu.cases(name)
    vals = m.cycle_values(*_cycle_of(cfg))
    masks = m.player_sign_masks(vals)
    L = len(vals)
    disc = np.float32(cfg["discount"])
    differs = 0
    for c in cases:
        A, K, _, sims = gu.dims(cfg, c)
        r = int(c["root_to_play"])
        depth = _tree_depths(c, K)
        tp = m.to_play_at_depth(r, depth, L)
        neg = np.array([bool((int(masks[r]) >> int((t - r) % L)) & 1) for t in tp])
        assert np.array_equal(neg, vals[tp] != vals[r])
        vs, plain = np.zeros(depth.size, np.float64), np.zeros(depth.size, np.float64)
        for s in range(sims):
            path = c["paths"][s][:c["path_len"][s]]
            v = float(c["tape_value"][s])
            for node in path[::-1]:
                vs[node] += -v if neg[node] else v
                plain[node] += v
                v = float(c["tree_reward"][node]) + float(disc) * v
        np.testing.assert_allclose(vs[1:], c["tree_value_sum"][1:], rtol=1e-4, atol=1e-3)
        differs += int(not np.allclose(plain[1:], c["tree_value_sum"][1:], rtol=1e-4, atol=1e-3))
    assert 2 * differs >= len(cases)


def test_game_fixture_roots_follow_the_move_number():
    cfg, data = gu.load("players/selfplay421_p2_sims10_T1")
    n = int(data["game_length"])
    assert np.array_equal(data["root_to_play"], np.arange(n) % int(cfg["number_of_player"]))


# ---- the kernels, cross-compiled (hipcc --offload-arch=gfx950 needs no GPU) ------------------------------------------------
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "stochastic-muzero_amd", "csrc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wno-unused-function", "-Wno-unused-variable",
         "-Wno-unused-const-variable", "-S", "--cuda-device-only"]


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"), reason="needs hipcc")
@pytest.mark.parametrize("source,fused", [("smz_kernels.hip", False), ("smz_fused.hip", True)])
def test_multi_player_kernels_are_instantiated(tmp_path, source, fused):
    """Every dispatch of k_expand_backup has a k_expand_backup_mp twin (same template arguments), and the plain kernels
    keep their names."""
    out = tmp_path / "k.s"
    r = subprocess.run([HIPCC, *FLAGS, "-o", str(out), source], cwd=CSRC, capture_output=True,
                       text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    names = {l.split(":")[0] for l in out.read_text().split("\n") if l.startswith("_Z") and l.split(";")[0].strip().endswith(":")}
    plain = sorted(n for n in names if n.startswith("_ZN12_GLOBAL__N_115k_expand_backup") or "15k_expand_backup" in n)
    mp = sorted(n for n in names if "18k_expand_backup_mp" in n)
    plain = [n for n in plain if "k_expand_backup_mp" not in n]
    assert plain and len(mp) == len(plain), (plain, mp)
    assert sorted(n.replace("18k_expand_backup_mp", "15k_expand_backup") for n in mp) == plain
    # the Philox specialisation of the fused kernel (A = 2 and 4, K = 2 and run-time) exists in both forms
    if fused:
        assert sum("Lb1ELb1ELb1E" in n for n in mp) == 4
