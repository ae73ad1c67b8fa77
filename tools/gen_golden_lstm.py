"""Golden vectors of the `lstm_model` head family, written by the reference itself.

TEST INFRASTRUCTURE.  Builds on oracle/gen_golden.py (run_case, save, export_state_dicts) and imports the reference through
oracle/_ref_import.py, so it runs only where the reference is available (SMZ_REFERENCE_DIR).  The tests read the committed
fixtures under tests/golden/lstm/ and nothing else.

  lstmnet_cartpole_L1.npz   a fresh reference net, CartPole-shaped (obs 4, A 2, S 31, H 64, L 1), torch seed 0
  lstmnet_lunar_L2.npz      a fresh reference net with two LSTM layers (obs 8, A 4, S 21, H 32, L 2), torch seed 1
      (state_dicts as flat "<function>/<key>" arrays + meta_*, the layout Muzero.from_state_dicts reads)
  lstm_cartpole_sims50.npz  16 reference searches with the first net (50 simulations, K 2), tree s under numpy seed s
  lstm_lunarL2_K2_sims30.npz 16 reference searches with the second net (30 simulations, K 2)
      (run_case's fields: the TapeModel tape of every network call, root statistics, the final tree, ...)

    python tools/gen_golden_lstm.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _ref_import as R  # noqa: E402
import gen_golden as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lstm")


def fresh_lstm(ref, obs_dim, A, S, H, L, seed):
    torch.manual_seed(seed)
    np_state = np.random.get_state()
    mz = ref.model.Muzero(model_structure="lstm_model", observation_space_dimensions=ref.Box(-1.0, 1.0, shape=(obs_dim,)),
                          action_space_dimensions=ref.Discrete(A), state_space_dimensions=S, hidden_layer_dimensions=H,
                          number_of_hidden_layer=L, k_hypothetical_steps=5, learning_rate=1e-3, device="cpu",
                          use_amp=False, scaler_on=False, num_of_epoch=10)
    np.random.set_state(np_state)
    return mz


def searches(ref, mz, name, obs_dim, obs_seed, kw, trees):
    cases = []
    for s in range(trees):
        obs = torch.tensor(np.random.RandomState(obs_seed + s).uniform(-0.05, 0.05, (1, obs_dim)).astype(np.float32))
        cases.append(G.run_case(ref, mz, obs, s, kw))
    out0, G.OUT = G.OUT, OUT
    try:
        G.save(name, {k: v for k, v in kw.items() if v is not None}, cases)
    finally:
        G.OUT = out0


def main():
    os.makedirs(OUT, exist_ok=True)
    ref = R.import_reference()
    torch.set_num_threads(1)
    base = dict(pb_c_base=19652, pb_c_init=1.25, discount=0.999, root_dirichlet_alpha=0.25, root_exploration_fraction=0.1,
                maxium_action_sample=2, number_of_player=1, custom_loop=None)
    cp = fresh_lstm(ref, 4, 2, S=31, H=64, L=1, seed=0)
    G.export_state_dicts(cp, os.path.join(OUT, "lstmnet_cartpole_L1.npz"), model_structure="lstm_model", A=2, S=31, H=64,
                         L=1, obs=4, torch_seed=0)
    searches(ref, cp, "lstm_cartpole_sims50", 4, 4000, dict(base, num_simulations=50), trees=16)
    ll = fresh_lstm(ref, 8, 4, S=21, H=32, L=2, seed=1)
    G.export_state_dicts(ll, os.path.join(OUT, "lstmnet_lunar_L2.npz"), model_structure="lstm_model", A=4, S=21, H=32,
                         L=2, obs=8, torch_seed=1)
    searches(ref, ll, "lstm_lunarL2_K2_sims30", 8, 4200, dict(base, num_simulations=30, discount=0.997), trees=16)


if __name__ == "__main__":
    main()
