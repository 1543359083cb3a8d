"""The three kinds of native test phase on ONE runner (sfx_runner_test_phase, sfx_runner_tsf_test_phase,
sfx_runner_phi_test_phase; the one lockstep driver in csrc/sfx_runner.inc): result, selections and sequence word are
shared by the kinds, staging record, device block and loss block are each kind's own.  SF, TSF, φ, then SF again from
the same initial W on one runner: the second SF phase equals the first bit for bit, and the TSF and the φ phase
equal the same phase run alone on a fresh runner; one training run afterwards still works.

The engine is tests/test_gpu_runner_phi_test_phase.py's narrow one with the TSF state beside the φ net (G = d,
K = 0), which serves the schedules "active", "tsf" and "phi".  E = 3, horizon 4, a deterministic env, a given
schedule.
"""
import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_phi_runner import T_, make_state
from tests.test_gpu_runner_phi_test_phase import A, D, N_S, initial_W, make_engine, make_loop

pytestmark = pytest.mark.gpu

E, HORIZON = 3, 4
HP = dict(gamma=0.85, beta=0.5, lasso=0.05, lr_w=2e-3, wd_w=1e-3, lr_omega=5e-3, wd_omega=1e-4, lr_omega_decay=0.01)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


class DetEnv:
    """Task e's stream depends only on (seed, e) and the actions it was given; row 1 ends at step 2."""

    def __init__(self, seed):
        self.seed = seed
        self.rng, self.t = [None] * E, [0] * E

    def reset(self, e):
        self.rng[e], self.t[e] = np.random.default_rng([self.seed, e]), 0
        return self.rng[e].standard_normal(N_S, dtype=np.float32)

    def step(self, e, a):
        g = self.rng[e]
        s1 = g.standard_normal(N_S, dtype=np.float32) + np.float32(0.05 * a)
        phi = g.random(D, dtype=np.float32)
        done = e == 1 and self.t[e] == 2
        self.t[e] += 1
        return s1, phi, float(phi[e % D] + np.float32(0.125) * np.float32(a % 3)), done


def explore(draws, seed):
    g = np.random.default_rng(700 + seed)
    shape = (E, HORIZON) if draws == 1 else (E, HORIZON, 2)
    return np.where(g.random(shape) <= 0.3, g.integers(0, A, shape), -1).astype(np.int32)


def run_phase(loop, kind, dev):
    """One phase of `kind` from that kind's initial rows; everything it returns and every row it moved."""
    W, Wb = (t.to(dev) for t in initial_W(E, D + 3, 11))
    loop.set_test_env(DetEnv(5))
    if kind == "sf":
        loop.set_schedule("active")
        out = loop.test_phase(W, horizon=HORIZON, explore=explore(1, 1), want_actions=True)
        state = [W]
    elif kind == "tsf":
        loop.set_schedule("tsf")
        g = torch.Generator().manual_seed(12)
        Om = torch.empty(E, T_ + 1).uniform_(-0.5, 0.5, generator=g).to(dev)
        mom = torch.zeros(E, 2 * (D + T_) + 2, device=dev)
        opt = np.arange(E, dtype=np.int64) * 3
        out = loop.tsf_test_phase(W, Om, mom, opt, HP, horizon=HORIZON, explore=explore(2, 2), want_actions=True)
        state = [W, Om, mom, torch.from_numpy(opt)]
    else:
        loop.set_schedule("phi", p_end=0.1)
        out = loop.phi_test_phase(W, Wb, horizon=HORIZON, explore=explore(1, 3), want_actions=True)
        state = [W, Wb]
    return [np.array(o) for o in out], [t.cpu().clone() for t in state]


def run_sequence(kinds, then_train=False):
    st = make_state("narrow")
    eng = make_engine(st, "narrow")
    eng.tsf_setup(D, 0)
    for t in range(T_):
        eng.tsf_load_g(t, st.g[t])
    eng.tsf_load_h(st.h)
    loop = make_loop(eng)
    try:
        res = [run_phase(loop, k, eng.device) for k in kinds]
        if then_train:
            loop.set_schedule("phi", p_end=0.1)
            loop.prefill(20)
            loop.set_task(2)
            loop.run(5)
            assert loop.stats()["env_steps"] == 5
        return res
    finally:
        loop.close()
        eng.close()


def same(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and len(a[1]) == len(b[1])
            and all(torch.equal(x, y) for x, y in zip(a[1], b[1])))


def test_three_kinds_of_phase_on_one_runner():
    mixed = run_sequence(["sf", "tsf", "phi", "sf"], then_train=True)
    for (ret, loss, steps, acts), state in mixed:
        assert steps.tolist() == [HORIZON, 3, HORIZON]  # row 1 ended at step 2
        assert (acts[0] >= 0).all() and (acts[1, :3] >= 0).all() and (acts[1, 3:] == -1).all()
        assert np.isfinite(loss).all() and not torch.equal(state[0], initial_W(E, D + 3, 11)[0])
    assert same(mixed[3], mixed[0])                       # returns, loss sums, steps, actions and W
    assert same(mixed[1], run_sequence(["tsf"])[0])
    assert same(mixed[2], run_sequence(["phi"])[0])
