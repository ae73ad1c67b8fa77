"""lstm_model head family: the package's re-declared modules (compat_lstm.py) and the batched torch evaluation
(heads.LstmTorchHeads) against vectors the reference's own classes produced (tools/gen_golden_lstm.py, tests/golden/lstm/).

CPU torch on both sides, identical ATen kernels and operation order for the batch-1 calls => 1e-6 (observed 0)."""
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stochastic_muzero_amd  # noqa: E402,F401

model_mod = import_module("stochastic-muzero_amd.model")
heads_mod = import_module("stochastic-muzero_amd.heads")
compat_lstm = import_module("stochastic-muzero_amd.compat_lstm")
TOL = 1e-6
NETS = {"lstmnet_cartpole_L1": "lstm_cartpole_sims50", "lstmnet_lunar_L2": "lstm_lunarL2_K2_sims30"}
_FUNCS = ("representation", "prediction", "afterstate_prediction", "afterstate_dynamics", "dynamics", "encoder")


def _path(name):
    return os.path.join(G.GOLDEN, "lstm", name + ".npz")


def _net(name):
    return model_mod.Muzero.from_state_dicts(_path(name))


def _assert_state_dicts(m, z):
    n = 0
    for f in _FUNCS:
        sd = getattr(m, f + "_function").state_dict()
        want = {k[len(f) + 1:]: z[k] for k in z.files if k.startswith(f + "/")}
        assert set(sd) == set(want), (f, set(sd) ^ set(want))
        for k, v in sd.items():
            assert np.array_equal(v.numpy(), want[k]), (f, k)
            n += 1
    return n


@pytest.mark.parametrize("name", sorted(NETS))
def test_fresh_construction_draws_the_references_initial_weights(name):
    """Same torch seed, same construction order (the Encoder's unused modules included) => the reference's parameters
    bit for bit, every state_dict key (the shared mid layer of the encoder shows up as repeated keys)."""
    z = np.load(_path(name))
    torch.manual_seed(int(z["meta_torch_seed"]))
    m = model_mod.Muzero(model_structure="lstm_model", observation_space_dimensions=int(z["meta_obs"]),
                         action_space_dimensions=int(z["meta_A"]), state_space_dimensions=int(z["meta_S"]),
                         hidden_layer_dimensions=int(z["meta_H"]), number_of_hidden_layer=int(z["meta_L"]), random_tag=0)
    assert type(m.dynamics_function) is compat_lstm.Dynamics_function
    assert _assert_state_dicts(m, z) > 40


def test_number_of_hidden_layer_must_be_at_least_one():
    with pytest.raises(ValueError, match="num_layers"):
        model_mod.Muzero(model_structure="lstm_model", observation_space_dimensions=4, action_space_dimensions=2,
                         number_of_hidden_layer=0)


@pytest.mark.parametrize("name", sorted(NETS))
def test_batch1_inference_calls_reproduce_the_reference_tape(name):
    """Every network call the reference made in its searches (TapeModel): the five *_inference methods."""
    m = _net(name)
    cfg, cases = G.cases("lstm/" + NETS[name])
    for c in cases:
        h0 = m.representation_function_inference(torch.from_numpy(c["obs"][None]))
        np.testing.assert_allclose(h0.numpy()[0], c["root_hidden"], atol=TOL, rtol=0)
        pol, v = m.prediction_function_inference(h0)
        np.testing.assert_allclose(pol[0], c["root_policy"], atol=TOL, rtol=0)
        np.testing.assert_allclose(v, c["root_value_net"], atol=TOL, rtol=0)
        for s in range(int(cfg["num_simulations"])):
            h = torch.from_numpy(c["tape_hidden_in"][s][None])
            a = int(c["tape_action"][s])
            if c["tape_branch"][s]:         # parent was a chance node: dynamics + prediction (mcts:333-337)
                r, hn = m.dynamics_function_inference(h, a)
                pol, v = m.prediction_function_inference(hn)
            else:                           # afterstate dynamics + afterstate prediction (mcts:338-342)
                r, hn = np.float32(0), m.afterstate_dynamics_function_inference(h, a)
                pol, v = m.afterstate_prediction_function_inference(hn)
            np.testing.assert_allclose(hn.numpy()[0], c["tape_hidden_out"][s], atol=TOL, rtol=0)
            np.testing.assert_allclose(r, c["tape_reward"][s], atol=TOL, rtol=0)
            np.testing.assert_allclose(pol[0], c["tape_policy"][s], atol=TOL, rtol=0)
            np.testing.assert_allclose(v, c["tape_value"][s], atol=TOL, rtol=0)


@pytest.mark.parametrize("name", sorted(NETS))
def test_batched_evaluation_treats_every_row_as_its_own_sequence(name):
    """LstmTorchHeads' trunks on 256 rows at once == 256 batch-1 calls of the modules (the reference's search), and ==
    nn.LSTM fed [1, B, H] (seq 1, batch B).  The modules called on the 2-D batch itself run ONE B-step sequence: row b
    then depends on rows 0..b-1 -- what ModuleHeads would compute for this family."""
    m = _net(name)
    A, S = m.action_dimension, m.state_dimension
    heads = heads_mod.LstmTorchHeads(*(getattr(m, f + "_function") for f in _FUNCS[:5]), num_actions=A, support_size=S,
                                     device="cpu")
    g = torch.Generator().manual_seed(1)
    B = 256
    x = torch.cat([torch.rand(B, S, generator=g), torch.nn.functional.one_hot(torch.randint(0, A, (B,), generator=g), A)], 1)
    seqs = [m.dynamics_function.reward, m.dynamics_function.next_state_normalized,
            m.afterstate_dynamics_function.next_state_normalized, m.prediction_function.policy, m.prediction_function.value,
            m.afterstate_prediction_function.policy, m.afterstate_prediction_function.value]
    with torch.no_grad():
        for t, seq in enumerate(seqs):
            xin = x if t < 3 else x[:, :S].contiguous()
            got = heads._trunk(t, xin)
            rows = torch.cat([seq(xin[i:i + 1]) for i in range(B)])
            torch.testing.assert_close(got, rows, atol=TOL, rtol=0)
            seq1 = seq[2](seq[1](seq[0](xin).unsqueeze(0)))[0]
            torch.testing.assert_close(got, seq1, atol=TOL, rtol=0)
            coupled = seq(xin)
            assert torch.equal(coupled[0], rows[0]) or torch.allclose(coupled[0], rows[0], atol=TOL)
            assert (coupled[1:] - rows[1:]).abs().max() > 1e-3          # the batch coupling of the 2-D call


def test_reference_class_paths_and_a_load_without_the_reference(tmp_path):
    """save_model writes whole-module pickles naming neural_network_lstm_model.* (the reference's checkpoint layout,
    muzero_model.py:911-949); a fresh interpreter without the reference on sys.path loads them through compat_lstm."""
    m = _net("lstmnet_lunar_L2")
    m.save_model(directory=str(tmp_path), tag=55)
    raw = open(os.path.join(tmp_path, "55_muzero_dynamics_function.pt"), "rb").read()
    assert b"neural_network_lstm_model" in raw and b"extract_tensor" in raw
    assert "neural_network_lstm_model" not in sys.modules
    m2 = model_mod.Muzero.from_checkpoint(str(tmp_path), tag=55)
    assert m2.model_structure == "lstm_model" and m2.action_dimension == 4 and m2.number_of_hidden_layer == 2
    assert type(m2.dynamics_function) is compat_lstm.Dynamics_function
    assert _assert_state_dicts(m2, np.load(_path("lstmnet_lunar_L2"))) > 40
    h = torch.rand(1, 21, generator=torch.Generator().manual_seed(0))
    assert torch.equal(m.afterstate_dynamics_function_inference(h, 3), m2.afterstate_dynamics_function_inference(h, 3))
    r, hn = m.dynamics_function_inference(h, 1)
    r2, hn2 = m2.dynamics_function_inference(h, 1)
    assert r == r2 and torch.equal(hn, hn2)
    assert np.array_equal(m.prediction_function_inference(h)[0], m2.prediction_function_inference(h)[0])
    m2.save_model(directory=str(tmp_path / "again"), tag=56)
    m3 = model_mod.Muzero.from_checkpoint(str(tmp_path / "again"), tag=56)
    assert _assert_state_dicts(m3, np.load(_path("lstmnet_lunar_L2"))) > 40
    code = ("import sys; sys.path.insert(0, %r); import stochastic_muzero_amd; from importlib import import_module; "
            "M = import_module('stochastic-muzero_amd.model'); m = M.Muzero.from_checkpoint(%r, tag=55); "
            "assert not any('reference' in p for p in sys.path); "
            "print(type(m.prediction_function).__module__, m.model_structure)") % (ROOT, str(tmp_path))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["neural_network_lstm_model", "lstm_model"]


def test_cli_builds_a_fresh_lstm_model_from_a_config():
    """muzero_cli's fresh-model path for a config whose "muzero" section asks for lstm_model: the reference's initial
    weights under the config's torch seed."""
    import muzero_cli
    z = np.load(_path("lstmnet_cartpole_L1"))
    mz = {"model_structure": "lstm_model", "state_space_dimensions": 31, "hidden_layer_dimensions": 64,
          "number_of_hidden_layer": 1, "load": False}
    torch.manual_seed(0)
    m = muzero_cli.fresh_model(mz, 4, 2, tag=7)
    assert m.model_structure == "lstm_model" and m.random_tag == 7
    _assert_state_dicts(m, z)
    with pytest.raises(AssertionError):
        muzero_cli.fresh_model(dict(mz, model_structure="transformer_model"), 4, 2, tag=7)
