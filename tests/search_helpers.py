"""What the GPU tests of the single-launch searches share (helper module, no tests): the package's modules, the random-stream
modes, and the bit-for-bit comparison of dumped trees and per-tree stream positions between two engines."""
from importlib import import_module

import numpy as np


def _pkg(name):
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd." + name)


def _lib():
    import stochastic_muzero_amd as smz
    return smz._lib


def _rng(name):
    return _lib().RNG_PHILOX if name == "philox" else _lib().RNG_MT19937_NUMPY


def _states(e, rng, trees):
    return [e.philox_position(i) if rng == "philox" else e.get_rng_state(i) for i in trees]


def _snapshot(e, rng, trees):
    return [e.dump_tree(i) for i in trees], _states(e, rng, trees)


def _same_dumps(da, db):
    for x, y in zip(da, db):
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k


def _same_states(sa, sb, rng):
    for x, y in zip(sa, sb):
        if rng == "philox":
            assert x == y
        else:
            assert np.array_equal(x[0], y[0]) and x[1] == y[1]
