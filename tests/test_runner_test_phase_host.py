"""Host-side pieces of the native test phase (NativeEnvLoop.test_phase / .train) that need no GPU: the
exploration schedule drawn from Python's ``random`` in the reference's order, and the positions of the test
phases inside SFDQN.train's loop (agents/sfdqn.py:102-123)."""
import random

import numpy as np
import pytest


def _reference_episodes(E, T, epsilon, n_actions):
    """SFDQN.get_test_action's two draws (agents/sfdqn.py:127-128), for E sequential episodes of T steps:
    ``random.random() <= test_epsilon`` and then ``random.randrange(n_actions)``."""
    out = []
    for _ in range(E):
        row = []
        for _ in range(T):
            if random.random() <= epsilon:
                row.append(random.randrange(n_actions))
            else:
                row.append(-1)
        out.append(row)
    return out


@pytest.mark.parametrize("epsilon", [0.0, 0.03, 1.0])
@pytest.mark.parametrize("seed", [0, 7])
def test_draw_test_schedule_is_the_lockstep_draw(epsilon, seed):
    from sfx import lockstep
    from sfx.runner import draw_test_schedule

    E, T, A = 5, 40, 9
    random.seed(seed)
    got = draw_test_schedule(E, T, epsilon, A)
    st_got = random.getstate()
    random.seed(seed)
    want = lockstep._draw_schedule(E, T, epsilon, A)
    assert got.dtype == np.int32 and got.shape == (E, T)
    assert got.tolist() == want
    # the same draws, and the same state afterwards, as E sequential reference episodes
    random.seed(seed)
    ref = _reference_episodes(E, T, epsilon, A)
    assert got.tolist() == ref
    assert st_got == random.getstate()
    if epsilon == 0.0:
        assert (got == -1).all()  # random.random() == 0.0 is not drawn under these seeds
    if epsilon == 1.0:
        assert (got >= 0).all() and (got < A).all()


def test_draw_test_schedule_shares_the_lockstep_function(monkeypatch):
    """One function, not a fork: a change of sfx.lockstep._draw_schedule is a change of draw_test_schedule."""
    from sfx import lockstep
    from sfx.runner import draw_test_schedule

    calls = []

    def fake(E, T, eps, A):
        calls.append((E, T, eps, A))
        return [[3] * T for _ in range(E)]

    monkeypatch.setattr(lockstep, "_draw_schedule", fake)
    out = draw_test_schedule(2, 3, 0.5, 4)
    assert calls == [(2, 3, 0.5, 4)] and out.tolist() == [[3, 3, 3], [3, 3, 3]]


@pytest.mark.parametrize("n", [1, 10, 25])
@pytest.mark.parametrize("n_test_ev", [1, 10])
def test_phase_positions(n, n_test_ev):
    from sfx.runner import test_phase_steps

    assert test_phase_steps(n, n_test_ev) == [t for t in range(n) if t % n_test_ev == 0]
