"""Head modules of the `lstm_model` family under the reference's class names.

As compat_mlp does for `mlp_model`: a reference checkpoint pickles whole modules that name
`neural_network_lstm_model.{Representation,Prediction,Afterstate_prediction,Afterstate_dynamics,Dynamics,Encoder}_function`
and `neural_network_lstm_model.extract_tensor`; model.py registers this module under that name so that such files load
where the reference's source is not installed.  Pickle restores each module's attribute dictionary onto the classes
below, so the attribute names used in forward() have to agree: `state_norm`, `reward`, `next_state_normalized`,
`policy`, `value`, `encoder`.

Architecture facts restated from neural_network_lstm_model.py:
  * representation: one Linear(obs, S), then the per-row min-max scaling;
  * every other head is a `Sequential(Linear(in, H), LSTM(H, O, num_layers=L), extract_tensor)` trunk, one per output
    (dynamics: reward logits (O = S) and next state (O = S, scaled); afterstate dynamics: next state; the two predictions:
    policy logits (O = A) and value logits (O = S));
  * the encoder is an ELU MLP (its BatchNorm / Dropout / Tanh / spare Linear modules are built and never used).
The trunks are called on 2-D tensors, which nn.LSTM reads as ONE unbatched sequence: batch-1 calls (the reference's
search) are a length-1 sequence from zero state.  forward() keeps that meaning; batched evaluation of many trees, each as
its own length-1 sequence, is heads.LstmTorchHeads / heads.HipLstmHeads.
"""
import torch
import torch.nn as nn


def scale_to_bound_action(x):
    """Row-wise (x - min) / (max - min), ranges below 1e-5 widened by 1e-5 (the same rule as compat_mlp's)."""
    lo = x.amin(dim=1, keepdim=True)
    span = x.amax(dim=1, keepdim=True) - lo
    span = torch.where(span < 1e-5, span + 1e-5, span)
    return (x - lo) / span


class Onehot_argmax(torch.autograd.Function):
    """Straight-through one-hot of the arg-max (gradients pass unchanged)."""

    @staticmethod
    def forward(ctx, x):
        return torch.zeros_like(x).scatter_(-1, x.argmax(dim=-1, keepdim=True), 1.0)

    @staticmethod
    def backward(ctx, grad_output):
        return grad_output


class extract_tensor(nn.Module):
    """Keeps the output sequence of an nn.LSTM and drops its (h_n, c_n) state."""

    def forward(self, x):
        return x[0]


def _lstm_trunk(n_in, width, n_out, layers):
    return nn.Sequential(nn.Linear(n_in, width), nn.LSTM(width, n_out, layers), extract_tensor())


class Representation_function(nn.Module):
    def __init__(self, observation_space_dimensions, state_dimension, action_dimension, hidden_layer_dimensions,
                 number_of_hidden_layer):
        super().__init__()
        self.state_norm = nn.Linear(observation_space_dimensions, state_dimension)

    def forward(self, state):
        return scale_to_bound_action(self.state_norm(state))


class Dynamics_function(nn.Module):
    def __init__(self, state_dimension, action_dimension, observation_space_dimensions, hidden_layer_dimensions,
                 number_of_hidden_layer):
        super().__init__()
        self.action_space = action_dimension
        n_in = state_dimension + action_dimension
        self.reward = _lstm_trunk(n_in, hidden_layer_dimensions, state_dimension, number_of_hidden_layer)
        self.next_state_normalized = _lstm_trunk(n_in, hidden_layer_dimensions, state_dimension, number_of_hidden_layer)

    def forward(self, state_normalized, action):
        x = torch.cat([state_normalized, action], dim=1)
        return self.reward(x), scale_to_bound_action(self.next_state_normalized(x))


class Prediction_function(nn.Module):
    def __init__(self, state_dimension, action_dimension, observation_space_dimensions, hidden_layer_dimensions,
                 number_of_hidden_layer):
        super().__init__()
        self.policy = _lstm_trunk(state_dimension, hidden_layer_dimensions, action_dimension, number_of_hidden_layer)
        self.value = _lstm_trunk(state_dimension, hidden_layer_dimensions, state_dimension, number_of_hidden_layer)

    def forward(self, state_normalized):
        return self.policy(state_normalized), self.value(state_normalized)


class Afterstate_prediction_function(Prediction_function):
    pass


class Afterstate_dynamics_function(nn.Module):
    def __init__(self, state_dimension, action_dimension, observation_space_dimensions, hidden_layer_dimensions,
                 number_of_hidden_layer):
        super().__init__()
        self.action_space = action_dimension
        self.next_state_normalized = _lstm_trunk(state_dimension + action_dimension, hidden_layer_dimensions,
                                                 state_dimension, number_of_hidden_layer)

    def forward(self, state_normalized, action):
        return scale_to_bound_action(self.next_state_normalized(torch.cat([state_normalized, action], dim=1)))


class Encoder_function(nn.Module):
    """Chance-outcome encoder (training only; never called by the search).  Modules are created in the reference's
    order, the unused ones included, so that an equal torch seed draws the reference's initial weights."""

    def __init__(self, observation_space_dimensions, state_dimension, action_dimension, hidden_layer_dimensions,
                 number_of_hidden_layer):
        super().__init__()
        self.action_space = action_dimension
        first = nn.Linear(observation_space_dimensions, hidden_layer_dimensions)
        mid = nn.Linear(hidden_layer_dimensions, hidden_layer_dimensions)
        nn.Linear(hidden_layer_dimensions, state_dimension)              # built, never used
        self.scale = nn.Tanh()
        nn.BatchNorm1d(observation_space_dimensions)                      # built, never used
        nn.BatchNorm1d(hidden_layer_dimensions)
        nn.Dropout(0.1)
        act = nn.ELU()
        layers = [first, act] + [mid, act] * number_of_hidden_layer
        self.encoder = nn.Sequential(*layers, nn.Linear(hidden_layer_dimensions, action_dimension))

    def forward(self, o_i):
        c_e_t = torch.softmax(self.encoder(o_i), dim=-1)
        return Onehot_argmax.apply(c_e_t), c_e_t
