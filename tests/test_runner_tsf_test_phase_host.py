"""Host side of the native runner's TSF test phase (no GPU): the exploration schedule's draws, ω's learning-rate
schedule, and NativeEnvLoop.train's dispatch to tsf_test_phase."""
import random
import warnings

import numpy as np
import pytest
import torch

A = 9


def sequential_draws(E, horizon, eps):
    """E sequential reference episodes: two get_test_action draws per step (agents/tsfdqn_sequential.py:377-381
    called at :404 and :407)."""
    def get_test_action():
        return random.randrange(A) if random.random() <= eps else -1

    return [[(get_test_action(), get_test_action()) for _ in range(horizon)] for _ in range(E)]


@pytest.mark.parametrize("eps", [0.0, 0.03, 1.0])
@pytest.mark.parametrize("seed", [3, 11])
def test_schedule_is_the_reference_draws(eps, seed):
    from sfx import lockstep
    from sfx.runner import draw_tsf_test_schedule

    E, horizon = 5, 40
    random.seed(seed)
    got = draw_tsf_test_schedule(E, horizon, eps, A)
    state = random.getstate()
    assert got.dtype == np.int32 and got.shape == (E, horizon, 2)
    random.seed(seed)
    ref = sequential_draws(E, horizon, eps)
    assert random.getstate() == state  # the same number of draws
    assert got.tolist() == [[list(p) for p in row] for row in ref]
    random.seed(seed)
    lock = lockstep._tsf_draw_schedule(E, horizon, eps, A, False)
    assert got.tolist() == [[[xa, xa1] for xa, xa1, _ in row] for row in lock]
    assert ((got >= -1) & (got < A)).all()
    if eps == 0.0:
        assert (got == -1).all()
    if eps == 1.0:
        assert (got >= 0).all()
    # diag: the binding's diagnostic draw is consumed too, as lockstep does for an agent that prints
    random.seed(seed)
    with_diag = draw_tsf_test_schedule(E, horizon, eps, A, diag=True)
    state_diag = random.getstate()
    random.seed(seed)
    lock = lockstep._tsf_draw_schedule(E, horizon, eps, A, True)
    assert random.getstate() == state_diag
    assert with_diag.tolist() == [[[xa, xa1] for xa, xa1, _ in row] for row in lock]


def test_schedule_is_one_function(monkeypatch):
    from sfx import lockstep
    from sfx.runner import draw_tsf_test_schedule

    monkeypatch.setattr(lockstep, "_tsf_draw_schedule",
                        lambda E, T, eps, n, diag: [[(4, -1, False)] * T for _ in range(E)])
    assert draw_tsf_test_schedule(2, 3, 0.5, A).tolist() == [[[4, -1]] * 3] * 2


def _lib_or_skip():
    try:
        from sfx import _lib
    except (ImportError, OSError) as e:  # as tests/test_abi.py loads it: no device needed
        pytest.skip(f"libsfx.so cannot be loaded: {e}")
    return _lib


@pytest.mark.parametrize("decay", [0.0, 1e-3, 0.01, 0.5])
@pytest.mark.parametrize("lr", [5e-3, 0.37])
def test_lr_omega_is_lambda_lr(decay, lr):
    fn = _lib_or_skip().lib.sfx_tsf_test_lr_omega
    p = torch.nn.Parameter(torch.zeros(1))
    optim = torch.optim.Adam([{"params": [p], "lr": 1e-3}, {"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr}])
    sched = torch.optim.lr_scheduler.LambdaLR(optim, [lambda epoch: 1 ** epoch, lambda epoch: (1 - decay) ** epoch])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scheduler.step() before optimizer.step(): only the lr is of interest
        for k in range(3001):
            want = np.float32(optim.param_groups[1]["lr"])
            got = fn(lr, decay, k)
            assert np.float32(got) == want and float(np.float32(got)) == got, (k, got, want)
            sched.step()
    assert optim.param_groups[0]["lr"] == 1e-3


def test_train_dispatches_to_the_tsf_phase():
    from sfx.runner import NativeEnvLoop, test_phase_steps

    class Stub:
        def __init__(self, schedule):
            self.schedule, self.log, self.t = schedule, [], 0

        def set_task(self, index):
            self.log.append(("task", index))
            self.t = 0

        def run(self, n):
            self.t += n

        def test_phase(self, W, **kw):
            self.log.append(("sf", self.t, W, kw))
            return (np.array([1.0, 3.0]),)

        def tsf_test_phase(self, W, **kw):
            self.log.append(("tsf", self.t, W, kw))
            return (np.array([2.0, 4.0]), None, None)

    kw = dict(Omega="Om", adam_state="M", opt_steps="opt", hp="hp", horizon=6)
    stub = Stub("tsf")
    data = NativeEnvLoop.train(stub, [0, 2], 25, "W", n_test_ev=10, **kw)
    want = [t + 1 for t in test_phase_steps(25, 10)]
    assert want == [1, 11, 21]
    for task in (0, 2):
        i = stub.log.index(("task", task))
        assert stub.log[i + 1:i + 4] == [("tsf", t, "W", kw) for t in want]
    assert len(stub.log) == 2 * 4 and stub.t == 25
    assert [float(v) for v in data] == [3.0] * 6 and all(isinstance(v, np.float32) for v in data)
    # the other schedules keep the SF agent's phase
    for sched in ("all", "active"):
        stub = Stub(sched)
        data = NativeEnvLoop.train(stub, 1, 25, "W", n_test_ev=10, horizon=6)
        assert [x[:2] for x in stub.log] == [("task", 0)] + [("sf", t) for t in want]
        assert [float(v) for v in data] == [2.0] * 3
