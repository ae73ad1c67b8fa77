"""The mask-based descent of the LDS-resident two-action search kernels (SMZ_SELECT_MASKS, csrc/smz_select_masks.hpp) against
the CPU oracle, every tree bit for bit, at the smallest shapes at which it can go wrong.

k_search_mlp<2, 2, 1, false, true, MSK, PHX, true> finds each round's path through the evaluated blocks from ballots instead
of a pointer chase: every lane keeps the lineage of its two blocks (l >> 1 and 32 + (l >> 1) of tree slot l & 1) in registers.
What can go wrong is in the hand-off of a new block's lineage, in the second pass (blocks from 32 on, ancestors in both ballots),
in waves with one tree or none, in switched-off tree slots, and in the fallback to the sequential descent -- none of which
needs the workload's 4096 trees.  The launcher gives a wavefront two trees (the geometry of the specialised instantiations) only
beyond 2048 trees; SMZ_SEARCH_TPW=2 selects it for the small batches here, and every case asserts through last_kernel() that
the LDS-resident instantiation ran.

The chain is tests/test_gpu_fullsize_parity.py's: the step-wise kernels record a net-output tape, the oracle replays it and
must ask for the same leaves, and the single-launch kernel on the same seeds must equal the oracle's trees, paths, MinMax
bounds and stream positions.  References are computed once per (weights, batch, simulations, word source) and only read.
"""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import golden_util as gu
from gpu_harness import dev
from test_gpu_fullsize_parity import ALPHA, DISCOUNT, FRAC, assert_engine_equals_oracle, oracle_replay, stepwise_tape

pytestmark = pytest.mark.gpu

KERNEL = "k_search_mlp<2, 2, 1, false, true, %s, %s, true>"
_REF = {}


def _mods():
    import stochastic_muzero_amd  # noqa: F401
    return import_module("stochastic-muzero_amd.mcts"), import_module("stochastic-muzero_amd.model")


def _reference(wname, seeds, sims, philox=False, lengths=False):
    """(model, observations, oracle trees after the replay of the step-wise tape[, path length of every descent])."""
    key = (wname, tuple(int(s) for s in seeds), sims, philox)
    if key not in _REF:
        _, model_mod = _mods()
        model = model_mod.Muzero.from_arrays(os.path.join(gu.GOLDEN, wname + ".npz"))
        B = len(seeds)
        obs = np.random.RandomState(0).uniform(-0.05, 0.05, (B, 4)).astype(np.float32)
        eng, trees, tape = stepwise_tape(model, obs, np.asarray(seeds, np.uint64), sims, 2, philox=philox)
        lens = None
        if lengths:        # oracle_replay's loop, keeping the length of the path every oracle descent recorded
            lens = np.zeros((B, sims), np.int32)
            for s, rec in enumerate(tape):
                for i in range(B):
                    _, _, act, flag = trees[i].select()
                    assert act == rec["action"][i] and flag == rec["branch"][i], (s, i)
                    lens[i, s] = len(trees[i].dump()["path"])
                    trees[i].expand_backup(rec["policy"][i], rec["value"][i], reward=rec["reward"][i], hidden=rec["hidden"][i])
        else:
            oracle_replay(trees, tape)
        assert_engine_equals_oracle(eng, trees, sims, prior_rtol=0)
        eng.close()
        _REF[key] = (model, obs, trees, lens)
    return _REF[key]


class _Subset:
    """The trees `idx` of an engine, numbered from 0 (assert_engine_equals_oracle walks range(len(trees)))."""

    def __init__(self, eng, idx):
        self.eng, self.idx, self.cfg = eng, list(idx), eng.cfg

    def root_stats(self):
        sel = torch.as_tensor(self.idx, device="cuda")
        return tuple(t.index_select(0, sel) for t in self.eng.root_stats())

    def dump_tree(self, i):
        return self.eng.dump_tree(self.idx[i])

    def get_rng_state(self, i):
        return self.eng.get_rng_state(self.idx[i])

    def philox_position(self, i):
        return self.eng.philox_position(self.idx[i])


def _single_launch(monkeypatch, wname, seeds, sims, philox=False, active=None, lengths=False):
    import stochastic_muzero_amd as smz
    mcts_mod, _ = _mods()
    model, obs, trees, lens = _reference(wname, seeds, sims, philox, lengths)
    B = len(seeds)
    monkeypatch.setenv("SMZ_SEARCH_TPW", "2")
    monkeypatch.delenv("SMZ_SEARCH_TLDS", raising=False)
    monkeypatch.delenv("SMZ_SEARCH_WAVES", raising=False)
    heads = model.heads("cuda:0", backend="hip")
    m = mcts_mod.BatchedMCTS(B, num_simulations=sims, maxium_action_sample=2, discount=DISCOUNT, root_dirichlet_alpha=ALPHA,
                             root_exploration_fraction=FRAC, use_graph=False, single_launch=True,
                             rng_mode=smz._lib.RNG_PHILOX if philox else smz._lib.RNG_MT19937_NUMPY)
    m.seed(np.asarray(seeds, np.uint64))
    if active is not None:
        m.set_active(dev(active.astype(np.uint8)))
    e = m.run(dev(obs), heads, train=True)
    torch.cuda.synchronize()
    assert m._single is True
    want = KERNEL % ("true" if (active is not None or philox) else "false", "true" if philox else "false")
    assert e.last_kernel() == want, e.last_kernel()
    if active is None:
        assert_engine_equals_oracle(e, trees, sims, prior_rtol=0)
    else:
        on = [i for i in range(B) if active[i]]
        assert_engine_equals_oracle(_Subset(e, on), [trees[i] for i in on], sims, prior_rtol=0)
    return lens


def _seeds(B):
    return np.arange(B, dtype=np.uint64) + 1000


# 1, 2: no expansion block yet in the first rounds; 31, 32: one pass; 33, 34: the first blocks of the second pass (a block from
# 32 on with ancestors in both ballots); 50: the workload's tree.  33 trees: 16 full waves, one wave with a single tree, and
# -- the third workgroup holds trees 32 .. 47 -- seven waves with none.
@pytest.mark.parametrize("sims", [1, 2, 31, 32, 33, 34, 50])
def test_every_tree_equals_the_oracle(sims, monkeypatch):
    _single_launch(monkeypatch, "weights_ckpt421", _seeds(33), sims)


def test_two_trees(monkeypatch):
    _single_launch(monkeypatch, "weights_ckpt421", _seeds(2), 50)


@pytest.mark.parametrize("off", ["every_second_tree", "one_whole_wave"])
def test_switched_off_trees(off, monkeypatch):
    """smz_set_active (the MSK instantiation): a wave whose one tree slot is off hands no lineage for it and its lanes contribute
    nothing to the ballots; a wave with both off leaves before the rounds."""
    B = 33
    active = np.ones(B, np.uint8)
    if off == "every_second_tree":
        active[1::2] = 0
    else:
        active[4:6] = 0                  # the third wave of the first workgroup
    _single_launch(monkeypatch, "weights_ckpt421", _seeds(B), 50, active=active)


@pytest.mark.parametrize("sims", [33, 50])
def test_philox_handle(sims, monkeypatch):
    _single_launch(monkeypatch, "weights_ckpt421", (np.arange(33, dtype=np.uint64) + np.uint64(7)) * np.uint64(0x9E3779B97F4A7C15),
                   sims, philox=True)


def test_paths_beyond_the_staged_words_take_the_sequential_descent(monkeypatch):
    """A block's pick is computed from the words its LEVEL reads, at a fixed offset in the 64 words staged for the round
    (select_words).  Levels 0 .. 20 read 64 words, and the round's expansion has drawn at least four words from the same window
    before the descent starts -- so a descent of 21 levels or more meets a block on its path that was not evaluated, the mask
    rule reports it, and that tree takes the sequential descent for the round while its wave partner does not.

    Checkpoint 421 gives paths of at most ~12 levels in 50 simulations.  tests/golden/weights_one_line.npz is that checkpoint with
    both policy heads replaced by the constant logits (+8, -8) and the value and reward heads zeroed: every search is nearly one
    line (chance levels still branch: their smoothed priors are 0.75 / 0.25).  The seeds were chosen on the CPU with the oracle
    (seven in the first 40000 reach 21 levels within 50 simulations); the test asserts from the path lengths the oracle records
    during the replay that such a descent is in the batch."""
    deep = [22999, 22200, 3033, 30263, 2802, 24760, 13894]
    seeds = np.array([1, deep[0], deep[1], 2, deep[2], deep[3], 3, deep[4], deep[5], deep[6], 4], np.uint64)
    lens = _single_launch(monkeypatch, "weights_one_line", seeds, 50, lengths=True)
    print("longest descent per tree:", lens.max(1))
    assert lens.max() >= 21 and (lens.max(1) >= 21).sum() >= 2, lens.max(1)
    assert lens.max(1).min() < 20                       # ... next to trees that never leave the block-parallel descent
