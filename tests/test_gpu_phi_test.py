"""GPU parity of the learned-φ agents' test phase in the library (sfx_phi_features, sfx_tsf_phi_test_action,
sfx_tsf_phi_test_update, sfx_phi_test_update; csrc/sfx_phitest.h): agents/tsfdqn_phi.py get_test_action /
update_target_models and agents/sfdqn_phi.py update_test_reward_mapper against

  * golden vectors from the real reference (tests/golden/test_{tsf_phi,phi}.npz, tools/gen_golden_phi_test.py);
  * tests/phi_test_ref.py (pinned by those vectors, tests/test_phi_test_golden.py) at small ragged shapes and
    at the full width of main_tsfdqn_phi_torch.py (hid 2048).

Tolerances as tests/test_gpu_tsf_phi.py: losses and λ 1e-4 relative, actions exact (after the test has asserted
that the restatement's top-2 gap of q is at least 1e-4 max |q|), parameters by params_close with
lr_steps = lr·k, at most 2e-3 of a group out (a fresh Adam's step is ±lr, so an entry whose gradient is at
rounding level may go the other way; the groups here have at most 768 entries: at most one, none below 500).
The seeds of CASES are those for which the fp32 restatement stays within that cap of its own float64 run:
test_phi_test_golden.py::test_small_case_seeds_fp32_vs_float64 checks it on the CPU."""
import ctypes
import math
import random
import types

import pytest
import torch

from tests import phi_test_ref as PT
from tests import tsf_phi_ref as TP
from tests.conftest import gpu_available
from tests.test_gpu_engine import params_close, rel_close

pytestmark = pytest.mark.gpu

GAMMA = 0.9


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


# ---- problems (CPU; shared with tests/test_phi_test_golden.py) --------------------------------
def small_problem(hid, T, A, d, seed):
    """Heads, φ net, g, h (tests/test_gpu_tsf_phi.py's problem; the target heads moved off the online ones) and
    a test task: Ω and b_w at torch's default Linear init, w ~ U(-0.5, 0.5), λ = 1."""
    from tests.test_gpu_tsf_phi import problem

    net = TP.Net(6, 64, A, d, ("relu", "relu"), hid, 3)
    st = problem(net, T, seed=seed, phi_init="torch" if hid > 1000 else "uniform")
    gen = torch.Generator().manual_seed(seed + 7)
    st.target = st.target + torch.empty_like(st.target).uniform_(-0.05, 0.05, generator=gen)
    return st, make_task(net, T, gen)


def make_task(net, T, gen):
    u = lambda *shape, a: torch.empty(*shape).uniform_(-a, a, generator=gen)
    Td = T * net.d
    return PT.TestTask(u(net.d, Td, a=1 / math.sqrt(Td)), u(net.d, a=1 / math.sqrt(Td)), u(net.d, a=0.5),
                       u(1, a=1 / math.sqrt(net.d)), torch.ones(1))



def chain(net, k, seed):
    """k chained transitions [(s, r, s1)] and a random action per step (for the SF-φ update)."""
    gen = torch.Generator().manual_seed(seed)
    s = torch.randn(net.n_s, generator=gen)
    out = []
    for _ in range(k):
        s1, r = torch.randn(net.n_s, generator=gen), float(torch.rand(1, generator=gen))
        out.append((s, r, s1, int(torch.randint(0, net.A, (1,), generator=gen))))
        s = s1
    return out


# (hid, T, A, d, seed): hid 131 has no vector loads, 26 and 8 run the narrow kernels (8 narrower than the
# 13-wide input); every T of {1, 3, 5}, A of {5, 9}, d of {3, 12}
CASES = [(136, 3, 9, 12, 31), (200, 5, 5, 3, 32), (131, 1, 9, 12, 33), (26, 3, 5, 12, 34), (8, 5, 9, 3, 35)]
K_SMALL = 6


def assert_fair(j, gap, qmax):
    assert gap >= 1e-4 * qmax, f"step {j}: the restatement's own top-2 gap {gap:.3e} is below 1e-4 max |q| {qmax:.3e}"


# ---- engine side ----------------------------------------------------------------------------
def engine_of(st, **kw):
    from tests.test_gpu_tsf_phi import engine_of as base

    return base(st, kw.pop("ev", 1000), **kw)


def dev_task(tt: PT.TestTask):
    return tt.to(dtype=torch.float32, device="cuda")


def gpu_tsf_step(eng, td: PT.TestTask, s, r, s1, gamma=GAMMA):
    a = eng.tsf_phi_test_action(s, td.omega_w, td.omega_b, td.w, td.wb)
    lo = eng.tsf_phi_test_update(s, a, r, s1, gamma, td.omega_w, td.omega_b, td.w, td.wb, td.lam)
    return a, lo


def check_task(td: PT.TestTask, tt: PT.TestTask, k, names=("omega_w", "omega_b", "w", "wb")):
    for name in names:
        params_close(getattr(td, name), getattr(tt, name), 1e-3 * k, max_bad_frac=2e-3)
    if "omega_w" in names:
        rel_close(td.lam, tt.lam, rtol=1e-4, atol=1e-7)


# ---- 1. the fixtures through the engine ------------------------------------------------------
def test_tsf_phi_fixture_through_engine(golden):
    g = golden("test_tsf_phi")
    st, tt0 = PT.problem_of(g)
    eng, td = engine_of(st), dev_task(tt0)
    ptrs = [x.data_ptr() for x in td.groups().values()]
    for j, (s, a, r, s1) in enumerate(PT.steps_of(g)):
        got, lo = gpu_tsf_step(eng, td, s, r, s1, float(g["gamma"]))
        assert got.dtype == torch.int64 and got.dim() == 0 and int(got) == a, (j, int(got), a)
        rel_close(lo.cpu(), g["losses"][j], rtol=1e-4, atol=1e-7)
    assert [x.data_ptr() for x in td.groups().values()] == ptrs
    check_task(td, PT.final_of(g, tt0), int(g["k"]))
    assert torch.equal(eng.phi_get(), st.phi)  # the test phase trains neither the φ net ...
    assert torch.equal(eng.tsf_get_h(), st.h) and torch.equal(eng.get_head(0, 0), st.online[0])  # ... nor h, ψ
    eng.close()


def test_phi_fixture_through_engine(golden):
    g = golden("test_phi")
    st, tt0 = PT.problem_of(g)
    eng, td = engine_of(st, tsf=False), dev_task(tt0)
    for j, (s, a, r, s1) in enumerate(PT.steps_of(g)):
        # SFDQN_PHI.get_test_action goes through GPI_w, which the library already has: the same action
        _, q, _, _ = eng.gpi(s.reshape(1, -1), w=td.w)
        q = q[0] + td.wb
        c = int(torch.argmax(q.max(dim=1).values))
        assert int(torch.argmax(q[c])) == a, j
        loss = eng.phi_test_update(s, a, r, s1, td.w, td.wb)
        assert loss.shape == (1,)
        rel_close(loss.cpu(), g["losses"][j], rtol=1e-4, atol=1e-7)
    check_task(td, PT.final_of(g, tt0), int(g["k"]), names=("w", "wb"))
    eng.close()


# ---- 2. small ragged shapes against the restatement ------------------------------------------
@pytest.mark.parametrize("hid,T,A,d,seed", CASES)
def test_small_shapes_vs_restatement(hid, T, A, d, seed):
    st, tt = small_problem(hid, T, A, d, seed)
    sf_t = tt.to()  # the SF-φ update's own reward model
    phi = "mul" if hid == 26 else "dims"
    eng, td, sf_d = engine_of(st, phi=phi), dev_task(tt), dev_task(sf_t)
    for j, (s, r, s1, a_sf) in enumerate(chain(st.net, K_SMALL, seed)):
        a, gap, qmax, ref = PT.tsf_step(st, tt, s, r, s1, GAMMA)
        assert_fair(j, gap, qmax)
        got, lo = gpu_tsf_step(eng, td, s, r, s1)
        assert int(got) == a, (j, int(got), a, gap)
        rel_close(lo.cpu(), list(ref), rtol=1e-4, atol=1e-7)
        ref_sf = PT.sf_update(st, sf_t, s, a_sf, r, s1)
        rel_close(eng.phi_test_update(s, a_sf, r, s1, sf_d.w, sf_d.wb).cpu(), [ref_sf], rtol=1e-4, atol=1e-7)
    check_task(td, tt, K_SMALL)
    check_task(sf_d, sf_t, K_SMALL, names=("w", "wb"))
    eng.close()


# ---- 3. sfx_phi_features at full width --------------------------------------------------------
FULL = (2048, 4, 9, 12)


@pytest.fixture(scope="module")
def full():
    """The full-width problem (hid 2048, 12.6 M φ parameters, torch's default init), built once and left
    unchanged: every test takes copies."""
    st, tt = small_problem(*FULL, seed=41)
    return st, tt


def test_phi_features_full_width_vs_float64(full):
    st, _ = full
    net = st.net
    gen = torch.Generator().manual_seed(43)
    s, s1 = torch.randn(2, net.n_s, generator=gen), torch.randn(2, net.n_s, generator=gen)
    a = torch.randint(0, net.A, (2,), generator=gen)
    inp = torch.cat([s, a.reshape(2, 1).float(), s1], dim=1)
    ref32 = TP.phi_forward(st.phi, net, inp)
    ref64 = TP.phi_forward(st.phi.double(), net, inp.double())
    bound = max(2.0 * float((ref32.double() - ref64).abs().max()), 1e-6 * float(ref64.abs().max()))
    eng = engine_of(st)
    one = eng.phi_features(s[0], a[:1], s1[0]).cpu()   # the one-row kernels
    two = eng.phi_features(s, a, s1).cpu()             # the update's forward
    print(f"bound {bound:.3e}  B=1 max err {float((one[0].double() - ref64[0]).abs().max()):.3e}  "
          f"B=2 max err {float((two.double() - ref64).abs().max()):.3e}")
    assert one.shape == (1, net.d) and two.shape == (2, net.d)
    assert float((one[0].double() - ref64[0]).abs().max()) <= bound
    assert float((two.double() - ref64).abs().max()) <= bound
    assert float((one[0] - ref32[0]).abs().max()) <= bound
    eng.close()


# ---- 4. determinism ---------------------------------------------------------------------------
def test_full_width_steps_are_deterministic(full):
    st, tt = full
    steps = chain(st.net, 4, 45)
    outs = []
    for _ in range(2):
        eng, td = engine_of(st), dev_task(tt)
        rec = []
        for s, r, s1, _ in steps:
            a, lo = gpu_tsf_step(eng, td, s, r, s1)
            rec += [a.cpu().reshape(1).float(), lo.cpu()]
        outs.append(rec + [x.cpu() for x in td.groups().values()])
        eng.close()
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert not torch.equal(outs[0][-5], tt.omega_w)


# ---- 5. interleaved with training updates -----------------------------------------------------
def test_interleaved_with_training_updates():
    """Training update, test step, training update on another policy, test step: the test calls see the
    post-update heads (the flipped slot), targets (synced every update here), φ net, g and h; and leave the
    training updates' results bit for bit what they are without them."""
    from tests.test_gpu_tsf_phi import batch, gpu_state, update

    st, tt = small_problem(136, 3, 9, 12, seed=51)
    net, T = st.net, 3
    gen = torch.Generator().manual_seed(52)
    bs = [batch(net, 16, gen) for _ in range(2)]
    steps = chain(net, 2, 53)
    eng, plain, td = engine_of(st, ev=1), engine_of(st, ev=1), dev_task(tt)
    los = []
    for j, (i, b) in enumerate(zip((1, 2), bs)):
        TP.update(st, b, i, use_gpi=True, target_update_ev=1)
        los.append((update(eng, i, b, True).cpu(), update(plain, i, b, True).cpu()))
        s, r, s1, _ = steps[j]
        a, gap, qmax, ref = PT.tsf_step(st, tt, s, r, s1, GAMMA)
        assert_fair(j, gap, qmax)
        got, lo = gpu_tsf_step(eng, td, s, r, s1)
        assert int(got) == a, (j, int(got), a, gap)
        rel_close(lo.cpu(), list(ref), rtol=1e-4, atol=1e-7)
    check_task(td, tt, 2)
    for x, y in los:
        assert torch.equal(x, y)
    a, b = gpu_state(eng, T), gpu_state(plain, T)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    eng.close()
    plain.close()


# ---- 6. error paths ---------------------------------------------------------------------------
def test_error_paths():
    from sfx._lib import lib
    from sfx.engine import SFEngine

    st, tt = small_problem(136, 2, 9, 12, seed=61)
    net, td = st.net, dev_task(tt)
    s = torch.randn(net.n_s, device="cuda")
    a = torch.zeros((), dtype=torch.long, device="cuda")
    out = torch.empty(net.d, device="cuda")
    f = ctypes.c_float
    p = lambda t: t.data_ptr()

    def calls(eng, s_ptr=p(s)):
        h = eng.handle
        return dict(
            features=lambda: lib.sfx_phi_features(h, s_ptr, p(a), p(s), 1, p(out)),
            sf_update=lambda: lib.sfx_phi_test_update(h, s_ptr, p(a), f(0.5), p(s), p(td.w), p(td.wb), p(out)),
            action=lambda: lib.sfx_tsf_phi_test_action(h, s_ptr, p(td.omega_w), p(td.omega_b), p(td.w), p(td.wb), p(a)),
            update=lambda: lib.sfx_tsf_phi_test_update(h, s_ptr, p(a), f(0.5), p(s), f(0.9), p(td.omega_w),
                                                       p(td.omega_b), p(td.w), p(td.wb), p(td.lam), p(out)))

    def fails(fn, text):
        rc, msg = fn(), lib.sfx_last_error().decode()
        assert rc == -1 and text in msg, (rc, msg)

    eng = engine_of(st, phi=None)  # g, h loaded, no φ setup
    for fn in calls(eng).values():
        fails(fn, "sfx_phi_setup")
    eng.close()
    eng = engine_of(st, tsf=False)  # a φ net, no sfx_tsf_setup
    for name in ("action", "update"):
        fails(calls(eng)[name], "sfx_tsf_setup")
    assert calls(eng)["features"]() == 0 and calls(eng)["sf_update"]() == 0  # these need no TSF setup
    for G, K in ((net.d + 4, 0), (net.d, 2)):
        eng.tsf_setup(G, K)
        for name in ("action", "update"):
            fails(calls(eng)[name], "G = d and K = 0")
    eng.tsf_setup(net.d, 0)
    for fn in calls(eng, s_ptr=None).values():
        fails(fn, "null")
    assert lib.sfx_phi_features(eng.handle, p(s), p(a), p(s), 33, p(out)) == -1  # B > max_batch
    assert "max_batch" in lib.sfx_last_error().decode()
    eng.close()
    eng = SFEngine(2, net.n_s, net.H, net.A, net.d, net.acts, max_batch=32)
    eng.shard_setup(4, 0)
    for fn in calls(eng).values():
        fails(fn, "unsharded")
    eng.close()


# ---- 7. the drop-in ---------------------------------------------------------------------------
class _Task:
    """tasks/task.py interface, enough for add_training_task."""

    def __init__(self, n_s, A, d, idx):
        self.n_s, self.A, self.d, self.idx = n_s, A, d, idx

    def action_count(self):
        return self.A

    def feature_dim(self):
        return self.d

    def encode_dim(self):
        return self.n_s

    def get_w(self):
        w = torch.zeros(self.d, 1)
        w[self.idx % self.d, 0] = 1.0
        return w


def _dropin_sf(cls, st, T, dev, monkeypatch):
    from sfx.dropin import _host
    from sfx.dropin.features.deep import _unflat_into
    from tests.golden.recipe import agent_psi_lambda

    monkeypatch.setattr(_host, "torch_device", lambda: dev)
    monkeypatch.setattr("sfx.dropin.features.deep.get_torch_device", lambda: dev)
    net = st.net
    sf = cls(pytorch_model_handle=agent_psi_lambda(net.H, net.acts, 1e-3, dev), use_true_reward=False)
    sf.reset()
    for t in range(T):
        sf.add_training_task(_Task(net.n_s, net.A, net.d, t))
    with torch.no_grad():
        for t in range(T):
            _unflat_into(sf.psi[t][0][0], st.online[t])
            _unflat_into(sf.psi[t][1][0], st.target[t])
    layers = []
    for j, (o, i) in enumerate(net.phi_dims):
        layers += [torch.nn.Linear(i, o)] + ([torch.nn.ReLU()] if j < len(net.phi_dims) - 1 else [])
    pm = torch.nn.Sequential(*layers).to(dev)
    _unflat_into(pm, st.phi)
    return sf, pm


def _linear(weight, bias, dev):
    m = torch.nn.Linear(weight.shape[1], weight.shape[0], bias=bias is not None).to(dev)
    with torch.no_grad():
        m.weight.copy_(weight)
        if bias is not None:
            m.bias.copy_(bias)
    return m


def test_dropin_tsf_phi_test_phase(golden, monkeypatch):
    """An agent with the attributes of agents/tsfdqn_phi.py that sfx.dropin.bind reads replays the fixture with
    no training update before it: the first test call loads the φ net, h and every g_t."""
    from sfx.dropin import bind
    from sfx.dropin.features.deep import _unflat_into
    from sfx.dropin.features.deep_tsf_phi import DeepSF_TSF_PHI

    dev = torch.device("cuda", 0)
    g = golden("test_tsf_phi")
    st, tt0 = PT.problem_of(g)
    net, T, k = st.net, int(g["T"]), int(g["k"])
    sf, pm = _dropin_sf(DeepSF_TSF_PHI, st, T, dev, monkeypatch)
    own = []

    class TSFDQN_PHI:  # the agent's own torch code, in outline: what the fallback runs
        def update_deep_models(self, *a):
            raise AssertionError("not bound")

        def test_agent(self, task, test_index):
            return "user test_agent"

        def _flat(self, s_enc, heads):
            return heads(s_enc).swapaxes(1, 2).flatten(start_dim=2)

        def get_test_action(self, s_enc, w):
            own.append("action")
            with torch.no_grad():
                if random.random() <= self.test_epsilon:
                    return torch.tensor(random.randrange(self.n_actions)).to(self.device)
                return torch.argmax(w(self.omegas(self._flat(s_enc, self.sf.get_successors))))

        def update_target_models(self, w_approx, lam, r, s_enc, a, s1_enc):
            own.append("update")
            params = list(w_approx.parameters()) + list(self.omegas.parameters())
            opt = torch.optim.Adam([{"params": params}, {"params": [lam], "maximize": True}], lr=1e-3)
            phi = self.phi[0][0](torch.cat([s_enc.flatten(), a.flatten().float(), s1_enc.flatten()]))
            cat = lambda x: self.omegas(torch.cat([gf(x) for gf in self.g_functions]).flatten())
            tphi = phi * (self.h_function(cat(s_enc)) + self.h_function(cat(s1_enc)))
            psi_loss = torch.nn.functional.mse_loss(
                self.omegas(self._flat(s_enc, self.sf.get_successors)),
                tphi + self.gamma * self.omegas(self._flat(s1_enc, self.sf.get_next_successors)))
            phi_loss = torch.nn.functional.mse_loss(w_approx(tphi), torch.tensor([r], device=self.device))
            loss = phi_loss + lam * psi_loss
            opt.zero_grad()
            loss.backward()
            opt.step()
            with torch.no_grad():
                lam.clamp_(1e-2, 1e6)
            return loss, psi_loss, phi_loss

    bind.patch("agents.tsfdqn_phi", types.SimpleNamespace(TSFDQN_PHI=TSFDQN_PHI))
    agent = TSFDQN_PHI()
    agent.sf, agent.device, agent.gamma, agent.test_epsilon, agent.n_actions = sf, dev, float(g["gamma"]), 0.0, net.A
    agent.phi = ((pm, torch.nn.MSELoss(), None), (None, None, None))
    agent.g_functions = [torch.nn.Linear(net.n_s, net.d).to(dev) for _ in range(T)]
    agent.h_function = torch.nn.Linear(net.d, net.d).to(dev)
    for t in range(T):
        _unflat_into(agent.g_functions[t], st.g[t])
    _unflat_into(agent.h_function, st.h)
    agent.omegas = _linear(tt0.omega_w, tt0.omega_b, dev)
    w = _linear(tt0.w.reshape(1, -1), tt0.wb, dev)
    lam = torch.ones(1, requires_grad=True, device=dev)
    tensors = lambda: [agent.omegas.weight, agent.omegas.bias, w.weight, w.bias, lam]
    ptrs = [x.data_ptr() for x in tensors()]
    for j, (s, a, r, s1) in enumerate(PT.steps_of(g)):
        s_enc, s1_enc = s.reshape(1, -1).to(dev), s1.reshape(1, -1).to(dev)
        got = agent.get_test_action(s_enc, w)
        assert got.dtype == torch.int64 and got.dim() == 0 and got.device == dev and int(got) == a, (j, got, a)
        loss, psi_loss, phi_loss = agent.update_target_models(w, lam, r, s_enc, got, s1_enc)
        assert loss.shape == (1,) and psi_loss.dim() == 0 and phi_loss.dim() == 0
        rel_close(torch.stack([loss[0], psi_loss, phi_loss]).cpu(), g["losses"][j], rtol=1e-4, atol=1e-7)
    assert not own and [x.data_ptr() for x in tensors()] == ptrs  # the library ran, on the agent's own tensors
    got = PT.TestTask(*(x.detach().cpu().reshape(y.shape) for x, y in zip(tensors(), tt0.groups().values())))
    check_task(got, PT.final_of(g, tt0), k)
    # ε = 1: the action is Python's random under the seed, in the reference's order, and no library call
    def boom(*a, **k):
        raise AssertionError("a library call under ε = 1")

    sf._eng.tsf_phi_test_action = boom
    agent.test_epsilon = 1.0
    random.seed(5)
    acts = [int(agent.get_test_action(s_enc, w)) for _ in range(4)]
    random.seed(5)
    want = []
    for _ in range(4):
        random.random()
        want.append(random.randrange(net.A))
    assert acts == want and not own
    del sf._eng.tsf_phi_test_action
    agent.test_epsilon = 0.0
    # a re-created Ω (add_training_task does that) is picked up: the same step on a copy of the module
    tt = got.to()
    s, _, r, s1 = PT.steps_of(g)[0]
    s_enc, s1_enc = s.reshape(1, -1).to(dev), s1.reshape(1, -1).to(dev)
    agent.omegas = _linear(tt.omega_w, tt.omega_b, dev)
    a, gap, qmax, ref = PT.tsf_step(st, tt, s, r, s1, agent.gamma)
    assert_fair(0, gap, qmax)
    got_a = agent.get_test_action(s_enc, w)
    assert int(got_a) == a
    out = agent.update_target_models(w, lam, r, s_enc, got_a, s1_enc)
    rel_close(torch.stack([out[0][0], out[1], out[2]]).cpu(), list(ref), rtol=1e-4, atol=1e-7)
    params_close(agent.omegas.weight.detach(), tt.omega_w, 1e-3, max_bad_frac=2e-3)
    assert not own
    # a reward model without bias: the agent's own torch code, and still the restatement's numbers
    w_nb = _linear(tt.w.reshape(1, -1), None, dev)
    tt.wb.zero_()
    a, gap, qmax = PT.greedy(st, tt, s1)
    assert_fair(1, gap, qmax)
    ref = PT.tsf_update(st, tt, s1, a, 0.25, s, agent.gamma, train_bias=False)
    got_a = agent.get_test_action(s1_enc, w_nb)
    out = agent.update_target_models(w_nb, lam, 0.25, s1_enc, got_a, s_enc)
    assert own == ["action", "update"] and int(got_a) == a
    rel_close(torch.stack([out[0].reshape(()), out[1], out[2]]).detach().cpu(), list(ref), rtol=1e-4, atol=1e-7)
    params_close(w_nb.weight.detach().reshape(-1), tt.w, 1e-3, max_bad_frac=2e-3)
    params_close(agent.omegas.weight.detach(), tt.omega_w, 2e-3, max_bad_frac=2e-3)
    assert agent.test_agent(None, 0) == "user test_agent"


def test_dropin_phi_test_phase(golden, monkeypatch):
    """agents/sfdqn_phi.py's update_test_reward_mapper through sfx.dropin.bind, no training update before."""
    from sfx.dropin import bind
    from sfx.dropin.features.deep_phi import DeepSF_PHI

    dev = torch.device("cuda", 0)
    g = golden("test_phi")
    st, tt0 = PT.problem_of(g)
    net, T, k = st.net, int(g["T"]), int(g["k"])
    sf, pm = _dropin_sf(DeepSF_PHI, st, T, dev, monkeypatch)
    own = []

    class SFDQN_PHI:
        def test_agent(self, task, test_index):
            return "user test_agent"

        def update_test_reward_mapper(self, w_approx, r, s_enc, a, s1_enc):
            own.append("update")
            opt = torch.optim.Adam(w_approx.parameters(), lr=1e-3)
            phi = self.phi[0][0](torch.cat([s_enc.flatten(), a.flatten().float(), s1_enc.flatten()]))
            loss = torch.nn.functional.mse_loss(w_approx(phi), torch.tensor([r], device=self.device))
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss

    bind.patch("agents.sfdqn_phi", types.SimpleNamespace(SFDQN_PHI=SFDQN_PHI))
    agent = SFDQN_PHI()
    agent.sf, agent.device = sf, dev
    agent.phi = ((pm, torch.nn.MSELoss(), None), (None, None, None))
    w = _linear(tt0.w.reshape(1, -1), tt0.wb, dev)
    ptrs = [w.weight.data_ptr(), w.bias.data_ptr()]
    for j, (s, a, r, s1) in enumerate(PT.steps_of(g)):
        s_enc, s1_enc = s.reshape(1, -1).to(dev), s1.reshape(1, -1).to(dev)
        loss = agent.update_test_reward_mapper(w, r, s_enc, torch.tensor(a, device=dev), s1_enc)
        assert loss.dim() == 0
        rel_close([loss.item()], g["losses"][j], rtol=1e-4, atol=1e-7)
    assert not own and [w.weight.data_ptr(), w.bias.data_ptr()] == ptrs
    ref = PT.final_of(g, tt0)
    params_close(w.weight.detach().reshape(-1), ref.w, 1e-3 * k, max_bad_frac=2e-3)
    params_close(w.bias.detach(), ref.wb, 1e-3 * k, max_bad_frac=2e-3)
    # without bias: the agent's own method
    tt = PT.TestTask(tt0.omega_w, tt0.omega_b, ref.w.clone(), torch.zeros(1), tt0.lam)
    w_nb = _linear(tt.w.reshape(1, -1), None, dev)
    s, a, r, s1 = PT.steps_of(g)[0]
    want = PT.sf_update(st, tt, s, a, r, s1)
    loss = agent.update_test_reward_mapper(w_nb, r, s.reshape(1, -1).to(dev), torch.tensor(a, device=dev),
                                           s1.reshape(1, -1).to(dev))
    assert own == ["update"]
    rel_close([loss.item()], [want], rtol=1e-4, atol=1e-7)
    params_close(w_nb.weight.detach().reshape(-1), tt.w, 1e-3, max_bad_frac=2e-3)
