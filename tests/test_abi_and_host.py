"""CPU-side checks: the C-ABI library loads and exports every symbol include/smz.h declares (no compute without a
GPU), and the host-side mirrors of the reference's interfaces behave like the reference (goldens from
oracle/gen_golden.py)."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def test_library_exports_every_declared_symbol():
    import stochastic_muzero_amd as smz
    header = open(os.path.join(ROOT, "include", "smz.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*\*?(smz_\w+)\s*\(", header, flags=re.M))
    assert len(declared) >= 25
    assert declared == set(smz._lib.SIGNATURES), declared ^ set(smz._lib.SIGNATURES)
    lib = smz._lib.load()
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.smz_abi_version() == 1
    assert lib.smz_traj_floats(4, 2) == 4 + 3 * 2 + 3


def test_create_fails_loudly_without_a_gpu_or_with_bad_arguments():
    import stochastic_muzero_amd as smz
    lib = smz._lib.load()
    h = C.c_void_p()
    bad = smz._lib.Config(4, 2, 2, 3, 5, 0, 1.25, 0.95, 0.25, 0.25, 0, 0)      # pb_c_base = 0
    assert lib.smz_create(C.byref(bad), C.byref(h)) == smz._lib.SMZ_ERR_INVALID
    assert b"pb_c_base" in lib.smz_last_error()
    if not torch.cuda.is_available():
        ok = smz._lib.Config(4, 2, 2, 3, 5, 19652, 1.25, 0.95, 0.25, 0.25, 0, 0)
        assert lib.smz_create(C.byref(ok), C.byref(h)) == smz._lib.SMZ_ERR_HIP
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            smz.SearchEngine(4, 2, 3)


def test_search_object_keeps_the_reference_constructor_surface():
    """Monte_carlo_tree_search(**json) -- same kwargs, attributes, AssertionErrors (mcts:76-85, 148-173)."""
    mcts = _pkg("mcts")
    m = mcts.Monte_carlo_tree_search(pb_c_base=19652, pb_c_init=1.25, discount=0.999, root_dirichlet_alpha=0.25,
                                     root_exploration_fraction=0.1, num_simulations=11, maxium_action_sample=2,
                                     number_of_player=1, custom_loop=None)
    for k, v in dict(pb_c_base=19652, pb_c_init=1.25, discount=0.999, root_dirichlet_alpha=0.25,
                     root_exploration_fraction=0.1, num_simulations=11, maxium_action_sample=2, number_of_player=1,
                     custom_loop=None).items():
        assert getattr(m, k) == v
    m.cycle.global_reset()
    d = mcts.Monte_carlo_tree_search()
    assert (d.num_simulations, d.discount, d.maxium_action_sample) == (10, 0.95, 2)
    for bad in (dict(pb_c_base=0), dict(pb_c_base=1.5), dict(pb_c_init=1), dict(discount=-1.0),
                dict(root_dirichlet_alpha=2.0), dict(root_exploration_fraction=1.5), dict(num_simulations=-1),
                dict(num_simulations=2.0), dict(maxium_action_sample=0), dict(number_of_player=0), dict(custom_loop=3)):
        with pytest.raises(AssertionError):
            mcts.Monte_carlo_tree_search(**bad)
    b = mcts.BatchedMCTS(8, num_simulations=5)
    assert b.num_simulations == 5 and b.engine is None


def test_temperature_scheduler_matches_reference_table():
    sp = _pkg("selfplay")
    z = np.load(os.path.join(gu.GOLDEN, "temperature_schedule.npz"))
    modes = [str(m) for m in z["modes"]]
    for mi, epoch, actual, want in z["rows"]:
        got = sp.temperature_scheduler(int(epoch), int(actual), modes[int(mi)])
        got = np.nan if got is None else float(np.asarray(got).reshape(-1)[0])
        assert (np.isnan(want) and np.isnan(got)) or got == want, (modes[int(mi)], epoch, actual, got, want)
    assert sp.temperature_scheduler(10, 3, 0.35) == 0.35


@pytest.mark.parametrize("name", gu.SELFPLAY_FIXTURES)
def test_trajectory_chunk_to_game_records_and_priorities(name):
    """chunk_to_games rebuilds the lists of game.py:72-77 and make_priority reproduces what the reference's
    ReplayBuffer.save_game derived from the reference's own game (replay_buffer.py:109-137, game.py:316-337)."""
    sp = _pkg("selfplay")
    cfg, data = gu.load(name)
    T = int(data["game_length"]); A = 2; obs_dim = 4
    F = obs_dim + 3 * A + 3
    chunk = np.zeros((T, 1, F))
    chunk[:, 0, :4] = data["game_observations"]
    chunk[:, 0, 4] = data["game_rewards"]
    chunk[:, 0, 6:8] = data["game_policies"]
    chunk[:, 0, 8:10] = data["game_action_onehot"]
    chunk[:, 0, 10] = data["game_root_values"]
    chunk[:, 0, 11:13] = data["game_child_visits"]
    (g,) = sp.chunk_to_games(chunk, obs_dim, A, float(cfg["discount"]), priority_scale=0.5, limit_of_game_play=int(data["limit"]))
    assert g.game_length == T and g.done == bool(data["game_done"]) and g.reanalyzed is False
    assert all(o.shape == (1, 4) and o.dtype == torch.float32 for o in g.observations)
    assert np.array_equal(np.array(g.policies), data["game_policies"])
    assert np.array_equal(np.array(g.child_visits), data["game_child_visits"])
    assert np.array_equal(np.array(g.root_values, np.float32), data["game_root_values"])
    assert [int(np.argmax(a)) for a in g.action_history] == list(data["game_actions"])
    pos, top = g.make_priority(50)
    np.testing.assert_allclose(pos, data["buffer_prio_position"], rtol=1e-12)
    np.testing.assert_allclose(top, data["buffer_prio_game"], rtol=1e-12)
    # make_target (game.py:291-314) against the reference's own Game.make_target on the same game
    U, TD = int(data["target_unroll"]), int(data["target_td"])
    for i in range(T):
        tgt = g.make_target(i, U, TD)
        assert len(tgt) == U
        np.testing.assert_allclose([t[0] for t in tgt], data["target_values"][i], rtol=1e-12, atol=1e-12)
        assert [float(t[1]) for t in tgt] == list(data["target_rewards"][i])
        assert np.array_equal(np.array([t[2] for t in tgt]), data["target_policies"][i])


def test_checkpoint_surface_roundtrip(tmp_path):
    """save_model / load_model keep the reference's file names, JSON keys and pickled class paths
    (muzero_model.py:911-996)."""
    model = _pkg("model")
    m = model.Muzero.from_arrays(os.path.join(gu.GOLDEN, "weights_lunar_L2.npz"))
    m.save_model(directory=str(tmp_path), tag=77)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted([f"77_muzero_{f}_function.pt" for f in ("representation", "prediction", "afterstate_prediction",
                            "afterstate_dynamics", "dynamics", "encoder")] + ["77_muzero_init_variables.json"])
    import json
    iv = json.load(open(tmp_path / "77_muzero_init_variables.json"))
    for k in ("model_structure", "observation_space_dimensions", "action_space_dimensions", "state_space_dimensions",
              "k_hypothetical_steps", "learning_rate", "optimizer", "loss_type", "lr_scheduler", "num_of_epoch", "device",
              "hidden_layer_dimensions", "number_of_hidden_layer", "random_tag", "action_map", "use_amp",
              "priority_scale", "rescale_value_loss"):
        assert k in iv, k
    raw = open(tmp_path / "77_muzero_dynamics_function.pt", "rb").read()
    assert b"neural_network_mlp_model" in raw and b"Dynamics_function" in raw
    m2 = model.Muzero.from_checkpoint(str(tmp_path), tag=77)
    a1 = model.mlp_arrays_from_modules(m.representation_function, m.prediction_function, m.afterstate_prediction_function,
                                       m.afterstate_dynamics_function, m.dynamics_function)
    a2 = model.mlp_arrays_from_modules(m2.representation_function, m2.prediction_function, m2.afterstate_prediction_function,
                                       m2.afterstate_dynamics_function, m2.dynamics_function)
    assert all(torch.equal(a1[k], a2[k]) for k in a1)
    assert m2.action_dictionnary == [0, 1, 2, 3] and m2.state_dimension == 16 and m2.number_of_hidden_layer == 2


@pytest.mark.parametrize("name,wname", [("ckpt421_sims50", "weights_ckpt421"), ("lunarL2_K3_sims24", "weights_lunar_L2"),
                                        ("wideA11_K9_sims24", "weights_wide_A11"), ("ckpt450_sims11", "weights_ckpt450")])
def test_batch1_inference_api_reproduces_reference_outputs(name, wname):
    """The five *_inference methods (muzero_model.py:802-909) on CPU against the reference's recorded outputs.
    Same torch build, same float32 operations -> the hidden states and policies agree to 1e-6."""
    model = _pkg("model")
    m = model.Muzero.from_arrays(os.path.join(gu.GOLDEN, wname + ".npz"))
    cfg, cases = gu.cases(name)
    c = cases[0]
    h = m.representation_function_inference(torch.from_numpy(c["obs"][None]))
    np.testing.assert_allclose(h.numpy().ravel(), c["root_hidden"], atol=1e-6)
    p, v = m.prediction_function_inference(h)
    assert p.shape == (1, c["root_policy"].size) and p.dtype == np.float32 and isinstance(v, np.float32)
    np.testing.assert_allclose(p[0], c["root_policy"], atol=1e-6)
    for s in range(len(c["tape_branch"])):
        hin = torch.from_numpy(c["tape_hidden_in"][s][None])
        if c["tape_branch"][s]:
            r, h2 = m.dynamics_function_inference(hin, int(c["tape_action"][s]))
            p, v = m.prediction_function_inference(h2)
            np.testing.assert_allclose(r, c["tape_reward"][s], rtol=1e-4, atol=5e-4)
        else:
            h2 = m.afterstate_dynamics_function_inference(hin, int(c["tape_action"][s]))
            p, v = m.afterstate_prediction_function_inference(h2)
        np.testing.assert_allclose(h2.numpy().ravel(), c["tape_hidden_out"][s], atol=2e-6)
        np.testing.assert_allclose(p[0], c["tape_policy"][s], atol=1e-6)
        np.testing.assert_allclose(v, c["tape_value"][s], rtol=1e-4, atol=5e-4)


# module attributes that torch releases newer than the one the reference trained with add to every pickled nn.Module
# (torch.nn.Module.__setstate__ fills them in when a checkpoint lacks them)
_NEWER_MODULE_KEYS = ("_backward_pre_hooks", "_forward_hooks_with_kwargs", "_forward_hooks_always_called",
                      "_forward_pre_hooks_with_kwargs", "_state_dict_pre_hooks", "_load_state_dict_post_hooks")


def test_loads_the_reference_checkpoint_files_without_the_reference_source(tmp_path):
    """The 421 checkpoint in the reference's file layout AS AN OLDER TORCH WROTE IT (muzero_model.py:911-996): six
    whole-module pickles naming neural_network_mlp_model.* whose module state lacks the hook dictionaries newer torch
    releases add, an encoder without the onehot_argmax submodule, and an init_variables.json whose training settings differ
    from what save_model writes.  Built here from the committed array fixture, it loads through the compatibility classes
    while no module of the reference is importable, carries exactly those weights and evaluates like the array model."""
    import copy
    import json
    import sys
    model = _pkg("model")
    src = model.Muzero.from_arrays(os.path.join(gu.GOLDEN, "weights_ckpt421.npz"))
    src.random_tag = 421
    with model._compat_modules_bound(force=True):
        for f in model._FUNCS:
            mod = copy.deepcopy(getattr(src, f + "_function"))
            if f == "encoder":
                del mod.onehot_argmax
            for sub in mod.modules():
                for k in _NEWER_MODULE_KEYS:
                    sub.__dict__.pop(k, None)
            torch.save(mod, tmp_path / f"421_muzero_{f}_function.pt")
    iv = dict(src.init_variables(), lr_scheduler="cosineannealinglr", num_of_epoch=10000, priority_scale=0.5)
    (tmp_path / "421_muzero_init_variables.json").write_text(json.dumps(iv))
    for f in model._FUNCS:
        raw = open(tmp_path / f"421_muzero_{f}_function.pt", "rb").read()
        assert b"neural_network_mlp_model" in raw and f"{f.capitalize()}_function".encode() in raw, f
        assert not any(re.search(rb"(?<![A-Za-z])" + k.encode(), raw) for k in _NEWER_MODULE_KEYS), f   # (whole keys)
    assert b"StraightThroughEstimator" not in open(tmp_path / "421_muzero_encoder_function.pt", "rb").read()
    assert "neural_network_mlp_model" not in sys.modules
    m = model.Muzero.from_checkpoint(str(tmp_path), tag=421)
    assert "neural_network_mlp_model" not in sys.modules                # bound for the load only
    assert type(m.dynamics_function).__module__ == "neural_network_mlp_model"
    assert all(model._is_compat_class(type(getattr(m, f + "_function"))) for f in model._FUNCS)
    assert (m.extra["lr_scheduler"], m.extra["num_of_epoch"], m.extra["priority_scale"]) == ("cosineannealinglr", 10000, 0.5)
    got = model.mlp_arrays_from_modules(m.representation_function, m.prediction_function, m.afterstate_prediction_function,
                                        m.afterstate_dynamics_function, m.dynamics_function)
    z = np.load(os.path.join(gu.GOLDEN, "weights_ckpt421.npz"))
    for k, v in got.items():
        assert np.array_equal(v.numpy(), z[k]), k
    assert (m.observation_dimension, m.action_dimension, m.state_dimension) == (4, 2, 31)
    # the restored modules run: hooks dictionaries back in place, same numbers as the array model
    obs = torch.from_numpy(np.random.RandomState(0).uniform(-0.05, 0.05, (5, 4)).astype(np.float32))
    with torch.no_grad():
        h, h_src = m.representation_function(obs), src.representation_function(obs)
        assert torch.equal(h, h_src)
        for a, b in zip(m.prediction_function(h), src.prediction_function(h_src)):
            assert torch.equal(a, b)
        assert torch.equal(m.encoder_function(obs)[1], src.encoder_function(obs)[1])


def test_cli_argv_and_config_surface():
    """muzero_cli.py: modes and config path by substring (reference muzero_cli.py:13-25), JSON keys of the reference."""
    import sys
    sys.path.insert(0, ROOT)
    import muzero_cli
    modes, cfg, opts = muzero_cli.parse_argv(["muzero_cli.py", "train", "report", "play", "config/experiment_421_config.json"])
    assert cfg == "config/experiment_421_config.json"
    assert modes["train"] and modes["play"] and modes["report"] and not modes["benchmark"]
    modes, cfg, opts = muzero_cli.parse_argv(["muzero_cli.py", "BENCHMARK", "x/config_a.json", "--envs", "64"])
    assert modes["benchmark"] and not modes["train"] and opts["envs"] == 64
    with pytest.raises(Exception):
        muzero_cli.parse_argv(["muzero_cli.py", "train"])
    with pytest.raises(Exception):
        muzero_cli.parse_argv(["muzero_cli.py", "config/a.json"])
    config = {"monte_carlo_tree_search": {"pb_c_base": 19652, "pb_c_init": 1.25, "discount": 0.999,
                                          "root_dirichlet_alpha": 0.25, "root_exploration_fraction": 0.1,
                                          "num_simulations": 11, "maxium_action_sample": 2, "number_of_player": 1,
                                          "custom_loop": None}}
    kw = muzero_cli.mcts_kwargs(config)
    _pkg("mcts").Monte_carlo_tree_search(**kw)
    assert muzero_cli.mcts_kwargs(config, 2)["num_simulations"] == 2


def test_compiled_host_cartpole_step_equals_the_python_env():
    """smz_host_cartpole_step (plain C on the host, no GPU) against envs.HostCartPole: same float64 Euler arithmetic,
    observation for observation; flags 1 (terminated) and 2 (stopped by the step limit)."""
    import ctypes as C
    import stochastic_muzero_amd as smz
    from importlib import import_module
    envs = import_module("stochastic-muzero_amd.envs")
    lib = smz._lib.load()
    B, T, limit = 6, 60, 40
    py = [envs.HostCartPole() for _ in range(B)]
    state = np.stack([e.reset(seed=100 + i)[0].astype(np.float64) * 0 + e.state for i, e in enumerate(py)])
    state = np.ascontiguousarray(state)
    obs = np.zeros((B, 4), np.float32); rew = np.zeros(B, np.float32); flag = np.zeros(B, np.uint8); cnt = np.zeros(B, np.int32)
    rs = np.random.RandomState(3)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    seen = set()
    for t in range(T):
        act = rs.randint(0, 2, B).astype(np.int32)
        assert lib.smz_host_cartpole_step(P(state), P(act), P(obs), P(rew), P(flag), P(cnt), limit, B) == 0
        for i, e in enumerate(py):
            o, r, term = e.step(int(act[i]))[:3]
            assert np.array_equal(o, obs[i]) and r == rew[i] == 1.0
            want = 2 if t + 1 == limit else (1 if term else 0)
            assert flag[i] == want, (t, i, flag[i], want)
            seen.add(int(flag[i]))
    assert seen == {0, 1, 2} and (cnt == T).all()


def test_rng_mode_auto_is_parity_mode_for_every_baseline_config_and_philox_above_the_crossover():
    """VERDICT r5 next #1c: "auto" (bench.py's default) keeps the reference's draws up to the single-launch crossover -- every
    BASELINE config is below it -- and switches to counter streams above; the constructor's own default stays parity mode."""
    import inspect
    from importlib import import_module
    m = import_module("stochastic-muzero_amd.mcts")
    L = import_module("stochastic-muzero_amd._lib")
    for trees in (1, 1024, 4096, m.SINGLE_LAUNCH_MAX_TREES):
        assert m.resolve_rng_mode("auto", trees) == L.RNG_MT19937_NUMPY
    for trees in (m.SINGLE_LAUNCH_MAX_TREES + 1, 32768, 262144, 1 << 20):
        assert m.resolve_rng_mode("auto", trees) == L.RNG_PHILOX
    assert m.resolve_rng_mode("mt19937", 1 << 20) == L.RNG_MT19937_NUMPY and m.resolve_rng_mode("philox", 1) == L.RNG_PHILOX
    assert m.resolve_rng_mode(L.RNG_PHILOX, 7) == L.RNG_PHILOX
    assert inspect.signature(m.BatchedMCTS.__init__).parameters["rng_mode"].default == L.RNG_MT19937_NUMPY
