"""Host logic of the SF-φ agent's lockstep test phase (sfx.lockstep.test_tasks_lockstep_phi) on the CPU: the
reference's sequential loop (agents/sfdqn_phi.py:211-212 over test_agent :234-261, restated in
tests/test_gpu_phi_lockstep.py's agent) and the lockstep rollout must draw the same random numbers, take the same
actions, fit the same reward models and log the same lines in the same order.  The GPU's part
(sfx_phi_test_actions, sfx_phi_test_updates) is stood in for by tests/phi_test_ref.py behind the engine
interface, row by row, so the one-row and the E-row calls agree bit for bit here as they do on the device;
tests/test_gpu_phi_lockstep.py runs the real ones."""
import random
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import phi_test_ref as PT
from tests import tsf_phi_ref as TP
from tests.test_gpu_phi_lockstep import A_, D_, T_, _agent_class, _Env, _Log, make_state

CPU = torch.device("cpu")


class _Engine:
    """The SF-φ test-phase calls of SFEngine over tests/phi_test_ref.py (fp32, CPU)."""
    device = CPU
    PHI_ROWS = 16  # SFEngine.PHI_ROWS
    max_batch = 4  # below PHI_ROWS: the groups are of 4

    def __init__(self, st):
        self.st, self.action_rows, self.update_rows, self.single = st, [], [], 0

    def q(self, s, w, wb):
        st = self.st
        with torch.no_grad():
            psi = torch.stack([TP.psi_forward(st.online[t], st.net, s.reshape(1, -1).float())[0] for t in range(T_)])
            return F.linear(psi, w.reshape(1, -1), wb.reshape(1))[..., 0]  # [T, A]

    def phi_test_update(self, s, a, r, s1, w, wb):
        self.single += 1
        return self._update(s, a, r, s1, w, wb)

    def _update(self, s, a, r, s1, w, wb):
        z = torch.zeros(1)
        tt = PT.TestTask(z, z, w, wb, torch.ones(1))  # w, wb stepped in place
        return PT.sf_update(self.st, tt, torch.as_tensor(s).float(), int(a), float(np.float32(float(r))),
                            torch.as_tensor(s1).float(), as_tensors=True).reshape(1)

    def phi_test_actions(self, S, W, Wb):
        assert S.shape[0] <= min(self.PHI_ROWS, self.max_batch) and W.shape == (S.shape[0], D_) and Wb.shape == (S.shape[0],)
        self.action_rows.append(S.shape[0])
        out = []
        for e in range(S.shape[0]):
            q = self.q(S[e], W[e], Wb[e])
            c = int(torch.argmax(q.max(dim=1).values))
            out.append([c, int(torch.argmax(q[c]))])
        return torch.tensor(out)

    def phi_test_updates(self, s, a, r, s1, W, Wb, losses=None):
        E = s.shape[0]
        assert a.dtype == torch.int64 and r.dtype == torch.float32 and a.shape == r.shape == (E,)
        self.update_rows.append(E)
        losses = torch.empty(E) if losses is None else losses
        for e in range(E):
            losses[e] = self._update(s[e], a[e], r[e], s1[e], W[e], Wb[e:e + 1])[0]
        return losses


class _SF:
    """The members of sfx's DeepSF_PHI that the test phase touches, over _Engine."""

    def __init__(self, st):
        self.eng, self.flushed, self.loaded = _Engine(st), 0, 0

    def _phi_engine(self, phi_model, batch):
        self.loaded += 1
        return self.eng

    def _flush(self):
        self.flushed += 1

    def _out_device(self):
        return CPU

    def phi_test_supported(self, phi_model, w):
        return isinstance(w, torch.nn.Linear) and w.bias is not None

    def phi_test_update(self, phi_model, w_approx, r, s_enc, a, s1_enc):
        return self.eng.phi_test_update(s_enc, a, float(r), s1_enc, w_approx.weight.data.reshape(-1),
                                        w_approx.bias.data).reshape(())

    def GPI_w(self, state, w):
        q = self.eng.q(torch.as_tensor(state), w.weight.detach().reshape(-1), w.bias.detach())[None]
        return q, torch.squeeze(torch.argmax(torch.max(q, dim=2).values, dim=1))


@pytest.fixture(scope="module")
def st():
    return make_state(20, 1, seed=91)  # left unchanged: the test phase trains nothing of it


def fresh(st, E, eps, steps=7, ends_at=None, bias=True):
    agent = _agent_class()()
    agent.sf, agent.device, agent.T, agent.test_epsilon, agent.n_actions = _SF(st), CPU, steps, eps, A_
    agent.phi = ((object(), None, None), (None, None, None))
    agent.encoding = lambda s: s
    agent.logger = _Log()
    torch.manual_seed(92)
    agent.test_tasks_weights = [torch.nn.Linear(D_, 1, bias=bias) for _ in range(E)]
    return agent, [_Env(60 + e, CPU, (ends_at or {}).get(e)) for e in range(E)]


def run_both(st, E, eps, seed=9, phases=2, **kw):
    from sfx.lockstep import test_tasks_lockstep_phi

    random.seed(seed)
    ref, tasks0 = fresh(st, E, eps, **kw)
    R0 = [[ref.test_agent(t, i) for i, t in enumerate(tasks0)] for _ in range(phases)]
    st0 = random.getstate()
    random.seed(seed)
    agent, tasks1 = fresh(st, E, eps, **kw)
    params = [(w.weight, w.bias) for w in agent.test_tasks_weights]
    R1 = [test_tasks_lockstep_phi(agent, tasks1) for _ in range(phases)]
    assert random.getstate() == st0  # the same draws, no more, no fewer
    assert R1 == R0
    assert [t.actions for t in tasks1] == [t.actions for t in tasks0]
    assert agent.logger.lines == ref.logger.lines and len(ref.logger.lines) == phases * E
    for (pw, pb), wa, wb in zip(params, agent.test_tasks_weights, ref.test_tasks_weights):
        assert wa.weight is pw and wa.bias is pb  # written back into the user's own parameters
        assert torch.equal(wa.weight, wb.weight) and torch.equal(wa.bias, wb.bias)
    return agent, ref, tasks1


@pytest.mark.parametrize("E,eps", [(1, 0.05), (3, 0.0), (4, 0.3), (6, 0.3), (9, 1.0)])
def test_lockstep_matches_the_sequential_loop(st, E, eps):
    steps, phases = 7, 2
    agent, ref, _ = run_both(st, E, eps, steps=steps, phases=phases)
    eng = agent.sf.eng
    groups = [min(4, E - e0) for e0 in range(0, E, 4)]  # consecutive groups of max_batch rows
    want = [n for _ in range(phases) for n in groups for _ in range(steps)]
    assert eng.action_rows == want and eng.update_rows == want and eng.single == 0
    assert agent.sf.flushed == phases and agent.sf.loaded == phases
    assert ref.sf.eng.single == phases * E * steps and not ref.sf.eng.update_rows
    assert not torch.equal(agent.test_tasks_weights[0].weight, fresh(st, 1, 0.0)[0].test_tasks_weights[0].weight)


def test_draws_are_taken_in_the_reference_order(st):
    """ε = 1: every action is Python's random under the seed, task 0's steps first, then task 1's."""
    from sfx.lockstep import test_tasks_lockstep_phi

    agent, tasks = fresh(st, 3, 1.0, steps=5)
    random.seed(4)
    test_tasks_lockstep_phi(agent, tasks)
    random.seed(4)
    want = []
    for _ in range(3):
        row = []
        for _ in range(5):
            random.random()
            row.append(random.randrange(A_))
        want.append(row)
    assert [t.actions for t in tasks] == want


def test_indices_select_the_reward_models(st):
    from sfx.lockstep import test_tasks_lockstep_phi

    agent, tasks = fresh(st, 3, 0.0)
    before = [w.weight.detach().clone() for w in agent.test_tasks_weights]
    random.seed(1)
    test_tasks_lockstep_phi(agent, [tasks[2]], [2])
    moved = [not torch.equal(w.weight, b) for w, b in zip(agent.test_tasks_weights, before)]
    assert moved == [False, False, True] and agent.logger.lines[0][2] == 2


def test_episodes_that_may_end_run_the_sequential_loop(st):
    agent, ref, tasks = run_both(st, 3, 0.2, ends_at={1: 3})
    assert not agent.sf.eng.action_rows and not agent.sf.eng.update_rows and agent.sf.flushed == 0
    assert [len(t.actions) for t in tasks] == [14, 6, 14]  # two phases; task 1 breaks at its done


def test_a_reward_model_the_library_refuses_runs_the_sequential_loop(st):
    from sfx.lockstep import test_tasks_lockstep_phi

    agent, tasks = fresh(st, 2, 0.0, bias=False)
    seen = []
    assert test_tasks_lockstep_phi(agent, tasks, sequential=lambda task, i: seen.append((task, i)) or 1.5) == [1.5, 1.5]
    assert seen == [(tasks[0], 0), (tasks[1], 1)] and not agent.sf.eng.action_rows and not agent.sf.loaded


def test_declared_endless_task_that_ends_warns_and_stops(st):
    from sfx.lockstep import test_tasks_lockstep_phi

    random.seed(2)
    ref, tasks0 = fresh(st, 3, 0.0, ends_at={2: 4})
    want = [ref.test_agent(t, i) for i, t in enumerate(tasks0)]
    random.seed(2)
    agent, tasks1 = fresh(st, 3, 0.0, ends_at={2: 4})
    with pytest.warns(RuntimeWarning, match="declared never to end"):
        got = test_tasks_lockstep_phi(agent, tasks1, episodes_end=False)
    assert got == want and len(tasks1[2].actions) == 4  # ε = 0: no draw depends on where task 2 ended
    assert agent.logger.lines == ref.logger.lines
    for wa, wb in zip(agent.test_tasks_weights, ref.test_tasks_weights):
        assert torch.equal(wa.weight, wb.weight) and torch.equal(wa.bias, wb.bias)
    assert agent.sf.eng.update_rows == [3, 3, 3, 3, 2, 2, 2]


def test_enable_routes_each_agent_to_its_rollout(st, monkeypatch):
    from sfx import lockstep

    hits = []
    for name in ("test_tasks_lockstep", "test_tasks_lockstep_tsf", "test_tasks_lockstep_phi"):
        monkeypatch.setattr(lockstep, name, lambda agent, tasks, *a, _n=name, **k: hits.append(_n) or [0.0] * len(tasks))
    phi, tasks = fresh(st, 2, 0.0)
    plain = types.SimpleNamespace(sf=types.SimpleNamespace(), train=None, test_agent=None)   # SFDQN: no φ net
    plain_phi_attr = types.SimpleNamespace(sf=types.SimpleNamespace(), phi=None, train=None, test_agent=None)
    tsf = types.SimpleNamespace(sf=phi.sf, phi=phi.phi, omegas=[], train=None, test_agent=None)  # TSF: Ω is shared
    for agent in (phi, plain, plain_phi_attr, tsf):
        agent.train = lambda *a, **k: None
        lockstep.enable(agent)
        agent.test_agent(tasks[0], 0)
    assert hits == ["test_tasks_lockstep_phi", "test_tasks_lockstep", "test_tasks_lockstep", "test_tasks_lockstep_tsf"]
    assert lockstep.phi_agent(phi) and not lockstep.phi_agent(plain) and not lockstep.phi_agent(tsf)


def test_enable_before_train_assigns_the_phi_net(st):
    """The reference's order: enable(agent) on a freshly built SFDQN_PHI, then agent.train(...).  The agent has
    no ``phi`` attribute until add_training_task assigns it inside train (agents/sfdqn_phi.py:43 only annotates
    it, :136 assigns it), so the rollout must not be fixed when enable() runs."""
    from sfx import lockstep

    random.seed(8)
    ref, tasks0 = fresh(st, 3, 0.2)
    want = [[ref.test_agent(t, i) for i, t in enumerate(tasks0)] for _ in range(2)]
    random.seed(8)
    agent, tasks1 = fresh(st, 3, 0.2)
    phi = agent.phi
    del agent.phi
    assert not hasattr(agent, "phi")

    def train(*a, **k):
        agent.phi = phi  # add_training_task
        return [[agent.test_agent(t, i) for i, t in enumerate(k["test_tasks"])] for _ in range(2)]

    agent.train = train
    lockstep.enable(agent)
    assert agent.train([], 0, test_tasks=tasks1) == want
    assert agent.sf.eng.update_rows == [3] * 14 and agent.sf.eng.single == 0  # the φ rollout, both phases
    assert agent.logger.lines == ref.logger.lines
    for wa, wb in zip(agent.test_tasks_weights, ref.test_tasks_weights):
        assert torch.equal(wa.weight, wb.weight) and torch.equal(wa.bias, wb.bias)


def test_enable_binds_the_phi_rollout_into_the_train_loop(st):
    from sfx import lockstep

    random.seed(6)
    ref, tasks0 = fresh(st, 3, 0.2)
    want = [ref.test_agent(t, i) for i, t in enumerate(tasks0)]
    random.seed(6)
    agent, tasks1 = fresh(st, 3, 0.2)
    agent.train = lambda *a, **k: [agent.test_agent(t, i) for i, t in enumerate(k["test_tasks"])]
    lockstep.enable(agent)
    assert agent.train([], 0, test_tasks=tasks1) == want
    assert agent.sf.eng.update_rows == [3] * 7 and agent.logger.lines == ref.logger.lines
