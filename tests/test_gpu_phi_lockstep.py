"""GPU checks of the SF-φ agent's lockstep test phase (csrc/sfx_phitest.h k_phiE_fwd / k_phiE_fwd_lds / k_phiE_narrow,
k_phi_test_steps, k_phi_test_act; sfx_phi_features_rows, sfx_phi_test_updates, sfx_phi_test_actions;
sfx.lockstep.test_tasks_lockstep_phi): agents/sfdqn_phi.py's test_agent (:234-261) for E test tasks at once.

The contract is equality with the sequential path, so the comparisons are ``torch.equal`` against the one-row
calls (sfx_phi_features at B = 1, sfx_phi_test_update, DeepSF_PHI.GPI_w's arithmetic) and, for the phase,
against the sequential loop over the bound methods.  The float64 bound of the φ rows is
test_gpu_phi_test.py::test_phi_features_full_width_vs_float64's: twice the fp32 restatement's own error
against float64 (from the reference, not from the code under test).  The updates' rtol 1e-5 is against
tests/phi_test_ref.py's sf_update run in float64, with a floor of one fp32 ulp of the largest pre-step parameter:
the step subtracts ±1e-3 from an fp32 w, so an entry that it cancels to near zero still carries the rounding of
the w it came from.

Shapes: T = 3, A = 5, d = 5, n_s = 4.  d odd: the last PHI1_R row group is partial; n_in = 9 odd: layer 0
takes the scalar loads."""
import random
import types

import numpy as np
import pytest
import torch

from sfx.engine import SFEngine
from tests import phi_test_ref as PT
from tests import tsf_phi_ref as TP
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

T_, A_, D_, NS_, H_ = 3, 5, 5, 4, 32
PHIE = SFEngine.PHI_ROWS  # csrc/sfx_phitest.h PHIE
ROWS = (1, 2, 3, 8, PHIE)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def make_state(hid, n_mid, seed=71, d=D_):
    from tests.test_gpu_tsf_phi import problem

    net = TP.Net(NS_, H_, A_, d, ("relu", "relu"), hid, n_mid)
    return problem(net, T_, seed=seed, phi_init="torch" if hid > 1000 else "uniform")


def engine_of(st, **kw):
    from tests.test_gpu_phi_test import engine_of as base

    return base(st, tsf=False, **kw)


def transitions(n, seed):
    gen = torch.Generator().manual_seed(seed)
    s, s1 = torch.randn(n, NS_, generator=gen), torch.randn(n, NS_, generator=gen)
    return s, torch.randint(0, A_, (n,), generator=gen), s1


# ---- 1. rows equal the one-row kernel, bit for bit --------------------------------------------
# (hid, n_mid): 131 odd K, scalar loads; 132 K4 = 33, the tail inside the first 64 lanes, with 0 and 2 middle
# layers; 520 K4 = 130, a wave's share crosses 64 lanes; 2048 a full trip; 64 the narrow net
@pytest.mark.parametrize("hid,n_mid", [(131, 1), (132, 0), (132, 2), (520, 1), (2048, 1), (64, 1)])
def test_rows_equal_the_one_row_kernel(hid, n_mid):
    st = make_state(hid, n_mid)
    net = st.net
    s, a, s1 = transitions(PHIE, 72)
    inp = torch.cat([s, a.reshape(-1, 1).float(), s1], dim=1)
    ref32 = TP.phi_forward(st.phi, net, inp)
    ref64 = TP.phi_forward(st.phi.double(), net, inp.double())
    bound = max(2.0 * float((ref32.double() - ref64).abs().max()), 1e-6 * float(ref64.abs().max()))
    eng = engine_of(st)
    one = torch.cat([eng.phi_features(s[e], a[e:e + 1], s1[e]).clone() for e in range(PHIE)]).cpu()
    err1 = float((one.double() - ref64).abs().max())
    for E in ROWS:
        rows = eng.phi_features_rows(s[:E], a[:E], s1[:E]).cpu()
        err = float((rows.double() - ref64[:E]).abs().max())
        print(f"hid {hid} n_mid {n_mid} E {E}: bound {bound:.3e} rows err {err:.3e} one-row err {err1:.3e}")
        assert rows.shape == (E, net.d)
        for e in range(E):
            assert torch.equal(rows[e], one[e]), (E, e, rows[e], one[e])
        assert err <= bound
    eng.close()


# ---- 2. E updates equal E single updates ------------------------------------------------------
@pytest.mark.parametrize("hid", [132, 64])
def test_updates_equal_single_updates(hid):
    st = make_state(hid, 1, seed=73)
    E = 8
    s, a, s1 = transitions(E, 74)
    gen = torch.Generator().manual_seed(75)
    W = torch.empty(E, D_).uniform_(-0.5, 0.5, generator=gen)
    Wb = torch.empty(E).uniform_(-0.4, 0.4, generator=gen)
    # away from w·φ + b (|.| < 3 here) so that no row's ρ is at rounding level by accident
    r = 5.0 + torch.rand(E, generator=gen)
    r[2] = 3.0e4        # ρ² ~ 1e9 while 2 ρ φ stays far inside the ±1e10 clamp
    W[5] = 0.0          # w·φ + b = r exactly: ρ = 0, zero gradient, no step
    Wb[5] = 0.5
    r[5] = 0.5
    st64 = st.to(dtype=torch.float64)
    want = []
    for e in range(E):
        tt = PT.TestTask(torch.zeros(1), torch.zeros(1), W[e].double(), Wb[e:e + 1].double(), torch.ones(1))
        loss = PT.sf_update(st64, tt, s[e].double(), int(a[e]), float(r[e]), s1[e].double())
        want.append((tt.w, tt.wb, loss))
    eng = engine_of(st)
    Wd, Wbd = W.cuda(), Wb.cuda()
    loss = eng.phi_test_updates(s, a, r, s1, Wd, Wbd).cpu()
    single = []
    for e in range(E):
        w1, b1 = W[e].cuda(), Wb[e:e + 1].cuda()
        l1 = eng.phi_test_update(s[e], a[e:e + 1], float(r[e]), s1[e], w1, b1).cpu()
        single.append((w1.cpu(), b1.cpu(), l1))
    Wd, Wbd = Wd.cpu(), Wbd.cpu()
    # one fp32 ulp of the largest pre-step parameter (3e-8 for |w| < 0.5, 6e-8 with row 5's bias of 0.5)
    floor = float(np.spacing(np.float32(max(float(W.abs().max()), float(Wb.abs().max())))))
    for e in range(E):
        w1, b1, l1 = single[e]
        print(f"row {e}: loss {float(loss[e]):.9e} single {float(l1):.9e} float64 {want[e][2]:.9e}")
        assert torch.equal(Wd[e], w1) and torch.equal(Wbd[e:e + 1], b1) and torch.equal(loss[e:e + 1], l1), e
        np.testing.assert_allclose(Wd[e].double().numpy(), want[e][0].numpy(), rtol=1e-5, atol=floor)
        np.testing.assert_allclose(Wbd[e:e + 1].double().numpy(), want[e][1].numpy(), rtol=1e-5, atol=floor)
        np.testing.assert_allclose(float(loss[e]), want[e][2], rtol=1e-5, atol=1e-12)
    assert float(loss[5]) == 0.0 and torch.equal(Wd[5], W[5]) and float(Wbd[5]) == 0.5
    assert float(loss[2]) > 1e8
    assert torch.equal(eng.phi_get(), st.phi)
    eng.close()


# ---- 3. the biased selection ------------------------------------------------------------------
def gpi_w_style(eng, S, W, Wb):
    """DeepSF_PHI.GPI_w and get_test_action's greedy branch row by row: eng.gpi's q, plus the bias, argmax."""
    qs, sel = [], []
    for e in range(S.shape[0]):
        _, q, _, _ = eng.gpi(S[e:e + 1], w=W[e])
        q = q + Wb[e].reshape(1, 1, 1)
        c = int(torch.argmax(torch.max(q, dim=2).values, dim=1))
        qs.append(q[0])
        sel.append([c, int(torch.argmax(q[:, c, :]))])
    return torch.stack(qs), torch.tensor(sel)


@pytest.mark.parametrize("d", [5, 8, 12])
def test_biased_selection_random_rows(d):
    """d = 5: sfx_gpi's row takes its scalar dot product, as k_phi_test_act always does.  d = 8 and 12 (the
    shipped shape): it takes the float4 one (d a multiple of 4, d <= 16, T A <= 256, w 16-byte aligned), whose
    fmaf order is the same: q must still be equal bit for bit."""
    st = make_state(132, 1, seed=76, d=d)
    eng = engine_of(st)
    E = 8
    gen = torch.Generator().manual_seed(77)
    S = torch.randn(E, NS_, generator=gen).cuda()
    W = torch.empty(E, d).uniform_(-0.5, 0.5, generator=gen).cuda()
    Wb = torch.empty(E).uniform_(-1.0, 1.0, generator=gen).cuda()
    assert d % 4 or all(W[e].data_ptr() % 16 == 0 for e in range(E))  # the rows the float4 path needs
    q_want, sel_want = gpi_w_style(eng, S, W, Wb)
    q = torch.empty(E, T_, A_, device="cuda")
    sel = eng.phi_test_actions(S, W, Wb, q_out=q)
    assert torch.equal(q, q_want) and torch.equal(sel.cpu(), sel_want)
    assert torch.equal(eng.phi_test_actions(S, W, Wb).cpu(), sel_want)  # without the q output
    eng.close()


def test_biased_selection_tie_made_by_the_bias():
    """Two q one ulp apart, the larger at the later index; a bias of 4 rounds both to 5: the first index wins,
    while the unbiased selection picks the later one.  ψ is pinned through the heads' output layer (zero
    weights, the values in the bias), w = e_0, so q[t, a] = ψ_t[a][0] exactly."""
    lo, hi, bias = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)), np.float32(4.0)
    assert hi > lo and np.float32(lo + bias) == np.float32(hi + bias) == np.float32(5.0)  # the property, on the CPU
    st = make_state(132, 1, seed=78)
    net = st.net
    n_out = net.A * net.d
    for t in range(T_):
        st.online[t, -(n_out * net.H + n_out):] = 0.0
    st.online[0, -n_out + 1 * net.d] = float(lo)   # ψ_0[a = 1][0]
    st.online[1, -n_out + 2 * net.d] = float(hi)   # ψ_1[a = 2][0]
    eng = engine_of(st)
    S = torch.randn(1, NS_).cuda()
    W = torch.zeros(1, D_, device="cuda")
    W[0, 0] = 1.0
    Wb = torch.full((1,), float(bias), device="cuda")
    q = torch.empty(1, T_, A_, device="cuda")
    sel = eng.phi_test_actions(S, W, Wb, q_out=q).cpu()
    q_want, sel_want = gpi_w_style(eng, S, W, Wb)
    assert torch.equal(q, q_want) and float(q[0, 0, 1]) == float(q[0, 1, 2]) == 5.0
    assert sel.tolist() == [[0, 1]] and torch.equal(sel, sel_want)
    assert eng.test_actions(S, W).cpu().tolist() == [[1, 2]]
    eng.close()


# ---- 4. the phase -------------------------------------------------------------------------------
class _Log:
    def __init__(self):
        self.lines = []

    def log_target_error_progress(self, d):
        self.lines.append(d)


def _agent_class():
    """agents/sfdqn_phi.py's test members (:223-305), bound by sfx.dropin.bind as the user's module is."""
    from sfx.dropin import bind

    class SFDQN_PHI:
        def get_test_action(self, s_enc, w):
            with torch.no_grad():
                if random.random() <= self.test_epsilon:
                    a = torch.tensor(random.randrange(self.n_actions)).to(self.device)
                else:
                    q, c = self.sf.GPI_w(s_enc, w)
                    q = q[:, c, :]
                    a = torch.argmax(q)
                return a

        def test_agent(self, task, test_index):
            R = 0.0
            w = self.test_tasks_weights[test_index]
            s_enc = self.encoding(task.initialize())
            accum_loss = 0
            for _ in range(self.T):
                a = self.get_test_action(s_enc, w)
                s1, r, done = task.transition(a)
                s1_enc = self.encoding(s1)
                accum_loss += self.update_test_reward_mapper(w, r, s_enc, a, s1_enc).item()
                s_enc = s1_enc
                R += r
                if done:
                    break
            self.logger.log_target_error_progress(self.get_target_reward_mapper_error(R, accum_loss, test_index, self.T))
            return R

        def update_test_reward_mapper(self, w_approx, r, s_enc, a, s1_enc):
            raise AssertionError("the bound method runs the library")

        def get_target_reward_mapper_error(self, r, loss, task_index, ts):
            return (r, loss, task_index)

    bind.patch("agents.sfdqn_phi", types.SimpleNamespace(SFDQN_PHI=SFDQN_PHI))
    return SFDQN_PHI


class _Env:
    """tools/test_phase.py's ActionEnv (deterministic, its own RNG, never ending) recording its actions."""

    def __init__(self, seed, dev, ends_at=None):
        from tools.test_phase import ActionEnv

        self.env, self.actions, self.ends_at = ActionEnv(NS_, A_, D_, seed, dev), [], ends_at
        self.episodes_never_end = ends_at is None

    def initialize(self):
        self.n = 0
        return self.env.initialize()

    def transition(self, a):
        assert torch.is_tensor(a) and a.dim() == 0 and a.dtype == torch.int64
        self.actions.append(int(a))
        self.n += 1
        s1, r, _ = self.env.transition(a)
        return s1, r, self.ends_at is not None and self.n % self.ends_at == 0


@pytest.fixture()
def phase(monkeypatch):
    """One drop-in DeepSF_PHI (hid 132) and a factory of fresh agents over it: (agent, tasks) with E test
    tasks whose reward models start from the same seed."""
    from sfx.dropin.features.deep_phi import DeepSF_PHI
    from tests.test_gpu_phi_test import _dropin_sf

    dev = torch.device("cuda", 0)
    st = make_state(132, 1, seed=79)
    sf, pm = _dropin_sf(DeepSF_PHI, st, T_, dev, monkeypatch)
    cls = _agent_class()

    def fresh(E, eps, steps=12, ends_at=None):
        agent = cls()
        agent.sf, agent.device, agent.T, agent.test_epsilon, agent.n_actions = sf, dev, steps, eps, A_
        agent.phi = ((pm, torch.nn.MSELoss(), None), (None, None, None))
        agent.encoding = lambda s: s
        agent.logger = _Log()
        torch.manual_seed(80)
        agent.test_tasks_weights = [torch.nn.Linear(D_, 1).to(dev) for _ in range(E)]
        tasks = [_Env(90 + e, dev, (ends_at or {}).get(e)) for e in range(E)]
        return agent, tasks

    fresh.sf, fresh.st = sf, st
    return fresh


def run_both(fresh, E, eps, seed=5, **kw):
    from sfx.lockstep import test_tasks_lockstep_phi

    random.seed(seed)
    ref, tasks0 = fresh(E, eps, **kw)
    R0 = [ref.test_agent(t, i) for i, t in enumerate(tasks0)]
    st0 = random.getstate()
    random.seed(seed)
    agent, tasks1 = fresh(E, eps, **kw)
    R1 = test_tasks_lockstep_phi(agent, tasks1)
    assert random.getstate() == st0
    assert R1 == R0
    assert [t.actions for t in tasks1] == [t.actions for t in tasks0]
    assert agent.logger.lines == ref.logger.lines and len(ref.logger.lines) == E
    for wa, wb in zip(agent.test_tasks_weights, ref.test_tasks_weights):
        assert torch.equal(wa.weight, wb.weight) and torch.equal(wa.bias, wb.bias)
    return agent, ref, tasks1


@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("eps", [0.0, 0.3])
def test_phase_equals_the_sequential_loop(phase, E, eps):
    agent, ref, tasks = run_both(phase, E, eps)
    assert all(len(t.actions) == 12 for t in tasks)
    w0 = torch.nn.Linear(D_, 1)
    assert not torch.equal(agent.test_tasks_weights[0].weight.cpu(), w0.weight)  # the reward models moved


# ---- 5. preconditions and errors ----------------------------------------------------------------
def test_episodes_that_may_end_run_the_sequential_loop(phase, monkeypatch):
    from sfx.engine import SFEngine

    calls, real = [], SFEngine.phi_test_updates
    monkeypatch.setattr(SFEngine, "phi_test_updates", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    _, _, tasks = run_both(phase, 3, 0.3, ends_at={1: 5})
    assert not calls and [len(t.actions) for t in tasks] == [12, 5, 12]  # the sequential loop, no lockstep launch
    run_both(phase, 2, 0.3)
    assert len(calls) == 12


def test_more_tasks_than_a_launch_holds_run_as_groups(phase):
    _, _, tasks = run_both(phase, PHIE + 1, 0.2, steps=4)
    assert len(tasks) == PHIE + 1 and all(len(t.actions) == 4 for t in tasks)


def test_phase_leaves_the_training_state_untouched(phase):
    from sfx.lockstep import test_tasks_lockstep_phi

    agent, tasks = phase(3, 0.1)
    sf = phase.sf
    eng = sf._phi_engine(agent.phi[0][0], 1)

    def state():
        out = [eng.phi_get()]
        for t in range(T_):
            m, v, step = eng.get_adam(t)
            out += [eng.get_head(t, 0), eng.get_head(t, 1), eng.get_w(t)[0], m, v, torch.tensor(step)]
        return out

    before = state()
    random.seed(3)
    test_tasks_lockstep_phi(agent, tasks)
    for x, y in zip(before, state()):
        assert torch.equal(torch.as_tensor(x).cpu(), torch.as_tensor(y).cpu())
    assert torch.equal(before[0], phase.st.phi)


def test_error_paths():
    from sfx._lib import lib
    from sfx.engine import SFEngine

    st = make_state(132, 1, seed=81)
    net = st.net
    E = 2
    S = torch.randn(E, NS_, device="cuda")
    a = torch.zeros(E, dtype=torch.long, device="cuda")
    r = torch.zeros(E, device="cuda")
    W, Wb = torch.zeros(E, D_, device="cuda"), torch.zeros(E, device="cuda")
    out = torch.empty(E, D_, device="cuda")
    sel = torch.empty(E, 2, dtype=torch.long, device="cuda")
    p = lambda t: t.data_ptr()

    def calls(eng, E=E, s_ptr=p(S), stride=D_):
        h = eng.handle
        return dict(
            rows=lambda: lib.sfx_phi_features_rows(h, s_ptr, p(a), p(S), E, p(out)),
            actions=lambda: lib.sfx_phi_test_actions(h, s_ptr, E, p(W), stride, p(Wb), None, p(sel)),
            updates=lambda: lib.sfx_phi_test_updates(h, E, s_ptr, p(a), p(r), p(S), p(W), stride, p(Wb), p(out)))

    def fails(fn, text):
        rc, msg = fn(), lib.sfx_last_error().decode()
        assert rc == -1 and text in msg, (rc, msg)

    eng = engine_of(st, phi=None)
    for fn in calls(eng).values():
        fails(fn, "sfx_phi_setup")
    eng.close()
    eng = engine_of(st, max_batch=8)
    for fn in calls(eng).values():
        assert fn() == 0
    for fn in calls(eng, s_ptr=None).values():
        fails(fn, "null")
    for bad in (0, PHIE + 1, 9):  # below 1, above PHIE, above max_batch
        for fn in calls(eng, E=bad).values():
            fails(fn, f"min({PHIE}, max_batch)")
    for name in ("actions", "updates"):
        fails(calls(eng, stride=D_ - 1)[name], "w_stride")
    eng.close()
    eng = SFEngine(2, net.n_s, net.H, net.A, net.d, net.acts, max_batch=32)
    eng.shard_setup(4, 0)
    for fn in calls(eng).values():
        fails(fn, "unsharded")
    eng.close()
