"""The closed loop of the learned-policy engines and the per-episode ledgers (tests/closed_loop_check.py: the learned
family, tools/gpu_fuzz_closed.py --learned): an MLP or a GRU cell, on the lane engine or the matrix engine, alone or as a
population with a partial last group, arg-max or softmax with an exploration coin, a value head, an episode ledger whose
ring wraps and a quality model, each under the config speed, per-lane speeds, a schedule and a LatencySpeedController, in
the four episode modes, on every impl, through step_policy and through select(commit=True) + step.  Every action is the
twin's answer at the replayed call site; every slab the launches report (features, scores, probs, values, hidden),
last_value, the controller's state after every operation, A.gae on every launch, every reward's quality term and the
ledger and quality records are the twins' bits.

Shapes: the smallest at which the listed failures can occur -- 64..192 lanes (a partial wave, more than one block) for
single nets, 300..600 lanes for populations (2 or 3 groups of 256, the last partial), V <= 18, fewer than 60 decisions,
widths and H on, next to and past the 32-row tile and the lane engine's 64."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

STATS, CASES = {}, {}


def _run_cell(cell):
    import closed_loop_check as K
    import gpu_fuzz_closed
    for mode in range(len(K.EP_MODES)):
        seed = cell + mode * len(K.LEARNED_CELLS)
        mm, _, key, case = gpu_fuzz_closed.run_learned_seed(seed, None, STATS)
        assert not mm, (K.describe_learned(case), len(mm), mm[:6])
        assert key == "/".join(K.LEARNED_CELLS[cell] + (K.EP_MODES[mode],))
        CASES[seed] = case


@pytest.mark.parametrize("cell", range(32))
def test_closed_loop_learned_cell(cell):
    _run_cell(cell)


def test_closed_loop_learned_slice_is_not_vacuous():
    """Folds the counters of the 32 cells above (a cell that has not run yet, runs here)."""
    import closed_loop_check as K
    for cell in range(len(K.LEARNED_CELLS)):
        if cell not in CASES:
            _run_cell(cell)
    assert len(CASES) == K.LEARNED_SLICE
    assert K.assert_non_vacuous_learned(STATS, list(CASES.values())) == []
