"""smz_search_mlp_players / smz_search_mlp_players_act: declared alike by the header, the library and the ctypes binding; the
Python layers carry the opt-in flag; every instantiation of k_search_mlp_players exists and needs no more scratch memory than the
generic k_search_mlp instantiation of its bucket plus the margin of the multi-player backup (the code objects' resource metadata;
no disassembly is read)."""
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
ENTRY_POINTS = ("smz_search_mlp_players", "smz_search_mlp_players_act")
FIELDS = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "agpr_count", "sgpr_count")


def _binding():
    import importlib.util
    spec = importlib.util.spec_from_file_location("smz_lib_only", os.path.join(ROOT, "stochastic-muzero_amd", "_lib.py"))
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    return lib


def test_header_and_binding_declare_the_players_search_entry_points():
    with open(os.path.join(ROOT, "include", "smz.h")) as f:
        h = f.read()
    assert re.search(r"\nint smz_search_mlp_players\(smz_handle \*h, const smz_mlp_desc \*desc, const float \*weights_dev, "
                     r"const float \*obs_dev, int train,\s+smz_stream stream\);", h)
    assert re.search(r"\nint smz_search_mlp_players_act\(smz_handle \*h, const smz_mlp_desc \*desc, const float \*weights_dev, "
                     r"const float \*obs_dev, int train,\s+double temperature, const double \*pow_table_host, int32_t \*action_dev, "
                     r"double \*policy_dev,\s+double \*child_visits_dev, float \*root_value_dev, smz_stream stream\);", h)
    lib = _binding()
    # the argument lists of smz_search_mlp / smz_search_mlp_act
    assert len(lib.SIGNATURES["smz_search_mlp_players"][1]) == len(lib.SIGNATURES["smz_search_mlp"][1]) == 6
    assert len(lib.SIGNATURES["smz_search_mlp_players_act"][1]) == len(lib.SIGNATURES["smz_search_mlp_act"][1]) == 12
    for name in ENTRY_POINTS:
        assert lib.SIGNATURES[name][1][1]._type_ is lib.MlpDesc


def test_the_library_exports_the_players_search_entry_points():
    so = os.path.join(ROOT, "stochastic-muzero_amd", "libsmz.so")
    if not os.path.exists(so):
        pytest.fail("libsmz.so is not built (python __graft_entry__.py build)")
    import ctypes
    lib = ctypes.CDLL(so)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_python_layers_accept_the_flag():
    """BatchedMCTS(players_single_launch=...) defaults to off; SearchEngine has search_mlp_players; the CLI passes the config key
    through and leaves a config without it alone."""
    import inspect
    import sys
    sys.path.insert(0, ROOT)
    import stochastic_muzero_amd  # noqa: F401
    from importlib import import_module
    mcts_mod, eng_mod = import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.engine")
    assert inspect.signature(mcts_mod.BatchedMCTS.__init__).parameters["players_single_launch"].default is False
    assert mcts_mod.BatchedMCTS(4, number_of_player=2).players_single_launch is False
    assert mcts_mod.BatchedMCTS(4, number_of_player=2, players_single_launch=True).players_single_launch is True
    assert list(inspect.signature(eng_mod.SearchEngine.search_mlp_players).parameters)[1:] == [
        "mlp_desc", "weights", "obs", "train", "act_temperature"]
    assert inspect.signature(eng_mod.SearchEngine.search_mlp_players).parameters["train"].default is True
    assert inspect.signature(eng_mod.SearchEngine.search_mlp_players).parameters["act_temperature"].default is None
    import muzero_cli
    block = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.997, root_dirichlet_alpha=0.25, root_exploration_fraction=0.25,
                 num_simulations=5, maxium_action_sample=2, number_of_player=2, custom_loop=None)
    assert "players_single_launch" not in muzero_cli.mcts_kwargs(dict(monte_carlo_tree_search=dict(block)))
    kw = muzero_cli.mcts_kwargs(dict(monte_carlo_tree_search=dict(block, players_single_launch=True)))
    assert kw["players_single_launch"] is True and mcts_mod.BatchedMCTS(4, **kw).players_single_launch is True


def _kernels(text, needle):
    meta = text[text.index("amdhsa.kernels:"):]
    seen = {}
    for k in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", k, re.M)
        if m is None or ".private_segment_fixed_size" not in k or needle not in m.group(1):
            continue
        seen[m.group(1)] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, k).group(1)) for f in FIELDS}
    return seen


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("SMZ_SKIP_ISA_TESTS"),
                    reason="needs hipcc (cross-compiles without a GPU)")
def test_players_search_kernels_exist_and_stay_within_the_generic_kernels_scratch(tmp_path):
    """All 20 instantiations (5 action buckets x KS {2, 0} x PHX {0, 1}) are in the code object.  For each (MAXA, KS) the scratch
    memory (private_segment_fixed_size) of the MT19937 instantiation is at most that of the generic single-player kernel it is
    modelled on, k_search_mlp<MAXA, KS, 1, false, false, true, false, false> of the same checkout, plus 10 %, rounded up to the
    next 16 bytes: the multi-player backup adds three per-lane values (sign mask, turn index, cycle length), which may cost a few
    slots but not a new spill region.

    Reported, not asserted (DESIGN.md 3.7 has the figures of this build): vector / scalar register counts and spill counts of every
    instantiation.  LDS is dynamic (sized on the host: players_lds)."""
    jobs = {"players": ["smz_mlp_players_search.hip"], "search": ["smz_search.hip"],
            "search_wide": ["smz_search_wide.hip"]}
    procs = {n: subprocess.Popen([HIPCC, *FLAGS, "-o", str(tmp_path / (n + ".s")), *args], cwd=CSRC, stdout=subprocess.DEVNULL,
                                 stderr=subprocess.PIPE, text=True) for n, args in jobs.items()}
    for n, p in procs.items():
        _, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (n, err[-2000:])
    new = _kernels((tmp_path / "players.s").read_text(), "k_search_mlp_players")
    generic = {}
    for n in ("search", "search_wide"):
        generic.update(_kernels((tmp_path / (n + ".s")).read_text(), "12k_search_mlpI"))
    for n, f in sorted(new.items()):
        print(n, f)

    def find(seen, tag):
        hits = [n for n in seen if tag in n]
        assert len(hits) == 1, (tag, sorted(seen))
        return seen[hits[0]]

    over = {}
    for bucket in (2, 4, 8, 16, 32):
        for ks in (2, 0):
            for philox in (0, 1):
                find(new, "k_search_mlp_playersILi%dELi%dELb%dEE" % (bucket, ks, philox))
            mine = find(new, "k_search_mlp_playersILi%dELi%dELb0EE" % (bucket, ks))["private_segment_fixed_size"]
            g = find(generic, "12k_search_mlpILi%dELi%dELi1ELb0ELb0ELb1ELb0ELb0EE" % (bucket, ks))
            print("generic", bucket, ks, g)
            bound = -(-(g["private_segment_fixed_size"] * 11) // 10)             # + 10 %, rounded up
            bound = (bound + 15) // 16 * 16
            if mine > bound:
                over[(bucket, ks)] = (mine, g["private_segment_fixed_size"], bound)
    assert len(new) == 20, sorted(new)
    assert not over, over
