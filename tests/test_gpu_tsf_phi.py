"""GPU parity of TSF-DQN with a learned φ (sfx_tsf_phi_update, sfx_phi_setup_dims): agents/tsfdqn_phi.py
TSFDQN_PHI.update_deep_models over features/deep_tsf_phi.py DeepSF_TSF_PHI against

  * golden vectors from the real reference (tests/golden/upd_tsf_phi_{gpi,nogpi}.npz,
    tools/gen_golden_tsf_phi.py).  Their φ net has hid = 136, so test_tsf_phi_update_vs_golden runs the WIDE
    kernels and the glue; the narrow kernels under the glue (hid 26, hid 8) are compared with the restatement
    only, never with reference vectors;
  * tests/tsf_phi_ref.py (pinned by those vectors, tests/test_tsf_phi_golden.py) at small ragged
    shapes -- hid 136 / B 32, hid 200 / B 7, hid 131 / B 19 (no vector loads), and the narrow kernels
    (hid 26) under the glue -- and at the full width of main_tsfdqn_phi_torch.py (hid 2048).

Tolerances as tests/test_gpu_phi.py: losses and λ 1e-4 relative, next actions exact, parameters by
params_close with lr_steps = lr·k (a fresh Adam's first step is ±lr for any gradient well above ε, so
an entry whose gradient is at rounding level may go the other way; at most 2e-3 of a group).
At full width only two updates, against float64: the fp32 reference itself drifts from float64
after that (flipped share of the φ net on the CPU: 0, 4.7e-6, 3.7e-4 after 1, 2, 3 updates)."""
import ctypes

import pytest
import torch

from tests import tsf_phi_ref as TP
from tests.conftest import gpu_available
from tests.test_gpu_engine import params_close, rel_close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def engine_of(st: TP.State, ev: int, max_batch=32, tsf=True, phi="dims"):
    from sfx.engine import SFEngine

    net, T = st.net, st.online.shape[0]
    eng = SFEngine(T, net.n_s, net.H, net.A, net.d, net.acts, max_batch=max_batch)
    eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
    eng.set_target_update_ev(ev)
    for t in range(T):
        eng.load_head(t, st.online[t], 0)
        eng.load_head(t, st.target[t], 1)
        eng.load_w(t, st.w[t])
    if phi == "dims":
        eng.phi_setup_dims(net.hid, net.n_mid, 1e-3)
    elif phi == "mul":
        eng.phi_setup(net.hid // (2 * net.n_s + 1), net.n_mid, 1e-3)
    if phi:
        eng.phi_load(st.phi)
    if tsf:
        eng.tsf_setup(net.d, 0)
        for t in range(T):
            eng.tsf_load_g(t, st.g[t])
        eng.tsf_load_h(st.h)
    # the reward-model biases and loss coefficients: caller-owned device scalars (the agent's tensors)
    eng.test_wb = st.wb.clone().float().to(eng.device)
    eng.test_lam = st.lam.clone().float().to(eng.device)
    return eng


def update(eng, i, b, use_gpi, next_actions=None, transform=True):
    s, a, r, s1, gamma = b
    fn = eng.tsf_phi_update if transform else eng.phi_update
    return fn(i, s, a, r, s1, gamma, eng.test_wb[i:i + 1], eng.test_lam[i:i + 1], use_gpi=use_gpi,
              next_actions=next_actions)


def gpu_state(eng, T, tsf=True):
    out = dict(online=torch.stack([eng.get_head(t, 0) for t in range(T)]),
               target=torch.stack([eng.get_head(t, 1) for t in range(T)]),
               w=torch.stack([eng.get_w(t)[0] for t in range(T)]), phi=eng.phi_get(), wb=eng.test_wb.cpu(),
               lam=eng.test_lam.cpu())
    if tsf:
        out.update(g=torch.stack([eng.tsf_get_g(t)[0] for t in range(T)]), h=eng.tsf_get_h())
    return out


def check_params(eng, st: TP.State, T, k, frac=2e-3, tsf=True):
    got = gpu_state(eng, T, tsf)
    for name in ("online", "target", "w", "phi") + (("g", "h") if tsf else ()):
        params_close(got[name], getattr(st, name), 1e-3 * k, max_bad_frac=frac)
    params_close(got["wb"], st.wb, 1e-3 * k)
    rel_close(got["lam"], st.lam, rtol=1e-6, atol=1e-7)


def problem(net: TP.Net, T, seed, phi_init="uniform"):
    from sfx.init import reference_heads

    online, w = reference_heads(T, net.n_s, net.H, net.A, net.d, net.acts, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    if phi_init == "uniform":
        phi0 = torch.empty(net.P_phi).uniform_(-0.15, 0.15, generator=gen)
    else:  # torch's default init of the reference's Sequential
        torch.manual_seed(seed + 2)
        phi0 = torch.cat([torch.cat([m.weight.detach().reshape(-1), m.bias.detach()])
                          for m in (torch.nn.Linear(i, o) for o, i in net.phi_dims)])
    u = lambda *shape, a=0.3: torch.empty(*shape).uniform_(-a, a, generator=gen)
    return TP.State(net, online.clone(), online.clone(), w.clone(), u(T), phi0, u(T, net.d * net.n_s + net.d),
                    u(net.d * net.d + net.d, a=0.4), torch.ones(T))


def batch(net: TP.Net, B, gen):
    s, s1 = torch.randn(B, net.n_s, generator=gen), torch.randn(B, net.n_s, generator=gen)
    a = torch.randint(0, net.A, (B,), generator=gen)
    r = torch.rand(B, 1, generator=gen)
    gamma = torch.where(torch.rand(B, generator=gen) < 0.1, 0.0, 0.9)
    return s, a, r, s1, gamma


@pytest.mark.parametrize("case", ["tsf_phi_gpi", "tsf_phi_nogpi"])
def test_tsf_phi_update_vs_golden(golden, case):
    g = golden("upd_" + case)
    st0 = TP.problem_of(g)
    T = int(g["T"])
    eng = engine_of(st0, int(g["target_update_ev"]))
    st = st0.to()
    nxt = torch.empty(32, dtype=torch.int64, device="cuda")
    for j, b in enumerate(TP.batches_of(g)):
        i = int(g["policies"][j])
        ref = TP.update(st, b, i, use_gpi=bool(g["use_gpi"]), target_update_ev=int(g["target_update_ev"]))
        lo = update(eng, i, b, bool(g["use_gpi"]), next_actions=nxt)
        assert torch.equal(nxt.cpu(), ref[4]), f"update {j}: next actions"
        rel_close(lo.cpu(), g["losses"][j], rtol=1e-4, atol=1e-7)
    check_params(eng, TP.final_of(g, st0), T, int(g["k"]))
    eng.close()


# (hid, B, φ setup, max_batch): hid 8 < n_in = 13 at B = max_batch (the kept input block is wider than a
# hidden layer's); B = 48 / 64 run the 3- and 4-tile instantiations of the wide kernels
SMALL = [(136, 32, "dims", 32), (200, 7, "dims", 32), (131, 19, "dims", 32), (26, 32, "mul", 32),
         (8, 32, "dims", 32), (136, 48, "dims", 64), (200, 64, "dims", 64)]


@pytest.mark.parametrize("hid,B,phi,max_batch", SMALL)
@pytest.mark.parametrize("transform", [True, False])
def test_small_shapes_vs_restatement(hid, B, phi, max_batch, transform):
    """5 updates at d = 12, n_s = 6 (n_in = 13): ragged batch rows, W rows / columns and d; hid 131 takes
    the scalar-load path, hid 26 and hid 8 the one-workgroup φ kernels (hid 8 through sfx_phi_setup_dims,
    narrower than the input).  transform=False: sfx_phi_update (DeepSF_PHI.update_successor) on the same
    net."""
    net = TP.Net(6, 64, 9, 12, ("relu", "relu"), hid, 3)
    T, k = 3, 5
    st = problem(net, T, seed=21 + hid)
    eng = engine_of(st, 3, max_batch=max_batch, tsf=transform, phi=phi)
    gen = torch.Generator().manual_seed(hid)
    nxt = torch.empty(B, dtype=torch.int64, device="cuda")
    for j in range(k):
        i, b = (2 * j) % T, batch(net, B, gen)
        ref = TP.update(st, b, i, use_gpi=j % 2 == 0, target_update_ev=3, transform=transform)
        lo = update(eng, i, b, j % 2 == 0, next_actions=nxt, transform=transform)
        assert torch.equal(nxt.cpu(), ref[4]), f"update {j}: next actions"
        rel_close(lo.cpu(), list(ref[:4]), rtol=1e-4, atol=1e-7)
    check_params(eng, st, T, k, tsf=transform)
    eng.close()


FULL = TP.Net(6, 256, 9, 12, ("relu", "relu"), 2048, 3)


def test_full_width_error_budget_vs_float64():
    """hid 2048 (12.6 M φ parameters), T = 4, B = 32, two updates: the GPU, the fp32 restatement and a
    float64 restatement following the fp32 actions.  Losses within 1e-5 relative of float64; per group the
    GPU's share of flipped entries (|x - ref64| > 1e-5 + 1e-4 |ref64|) at most max(2 × the fp32
    restatement's, 2e-4) -- the rule of tests/test_gpu_phi.py test_phi_error_budget_vs_float64."""
    net, T, B = FULL, 4, 32
    st = problem(net, T, seed=4, phi_init="torch")
    s64 = st.to(dtype=torch.float64)
    eng = engine_of(st, 3)
    gen = torch.Generator().manual_seed(5)
    for j in range(2):
        i, b = (3 * j) % T, batch(net, B, gen)
        l32 = TP.update(st, b, i, use_gpi=True, target_update_ev=3)
        b64 = tuple(x if x.dtype == torch.int64 else x.double() for x in b)
        l64 = TP.update(s64, b64, i, use_gpi=True, target_update_ev=3, next_actions=l32[4])
        lo = update(eng, i, b, True).cpu().double()
        print(f"update {j}: GPU {lo.tolist()} fp32 {l32[:4]} float64 {l64[:4]}")
        for q in range(4):
            ref = float(l64[q])
            assert abs(float(lo[q]) - ref) <= 1e-5 * abs(ref) + 1e-9, (j, q, float(lo[q]), ref)

    def flips(x, ref64):
        x = torch.as_tensor(x).double().cpu().reshape(-1)
        ref64 = ref64.reshape(-1)
        bad = (x - ref64).abs() > 1e-5 + 1e-4 * ref64.abs()
        return float(bad.double().mean()), float((x - ref64).abs().max())

    got = gpu_state(eng, T)
    for name in ("online", "target", "w", "phi", "g", "h", "wb"):
        (fg, mg), (fr, mr) = flips(got[name], getattr(s64, name)), flips(getattr(st, name), getattr(s64, name))
        print(f"{name:8s} flipped vs float64: GPU {fg:.2e}  fp32 restatement {fr:.2e}   max |diff| {mg:.2e} / {mr:.2e}")
        assert fg <= max(2.0 * fr, 2e-4), (name, fg, fr)
        assert mg <= 2.0 * 1e-3 * 2 + 1e-5, (name, mg)
    eng.close()


def test_full_width_is_deterministic():
    """Two engines, the same state and inputs: every parameter bit-identical after two updates (fixed
    reduction order, no floating-point atomics)."""
    net, T, B = FULL, 4, 32
    st = problem(net, T, seed=6, phi_init="torch")
    engs = [engine_of(st, 3), engine_of(st, 3)]
    gen = torch.Generator().manual_seed(7)
    bs = [batch(net, B, gen) for _ in range(2)]
    los = [[update(e, (3 * j) % T, b, True).cpu() for j, b in enumerate(bs)] for e in engs]
    assert all(torch.equal(x, y) for x, y in zip(*los))
    a, b = (gpu_state(e, T) for e in engs)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    assert not torch.equal(a["phi"], st.phi)
    for e in engs:
        e.close()


def test_setup_dims_equals_setup(golden):
    """sfx_phi_setup_dims(hid = 2 n_in) runs sfx_phi_setup(width_mul = 2)'s kernels: bit-identical over
    the upd_phi_gpi golden run."""
    from tests.test_gpu_phi import engine_of as phi_engine_of, update as phi_update
    from tests.test_oracle_golden import phi_batches, phi_problem

    g = golden("upd_phi_gpi")
    st0 = phi_problem(g)
    T, ev = int(g["T"]), int(g["target_update_ev"])
    e1 = phi_engine_of(st0, ev)
    e2 = phi_engine_of(st0, ev)
    e2.phi_setup_dims(2 * (2 * st0.spec.n_s + 1), st0.pspec.n_mid, 1e-3)
    assert e2.phi_numel == e1.phi_numel and e2.phi_cfg == dict(hid=70, n_mid=3, lr=1e-3)
    e2.phi_load(st0.phi)
    for j, (s, a, r, _, s1, gamma) in enumerate(phi_batches(g)):
        i = int(g["policies"][j])
        l1, l2 = (phi_update(e, i, s, a, r, s1, gamma, True).cpu() for e in (e1, e2))
        assert torch.equal(l1, l2), j
    a, b = gpu_state(e1, T, tsf=False), gpu_state(e2, T, tsf=False)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    e1.close()
    e2.close()


def test_error_paths():
    from sfx._lib import lib

    net = TP.Net(6, 64, 9, 12, ("relu", "relu"), 136, 3)
    st = problem(net, 2, seed=3)
    b = tuple(x.cuda() for x in batch(net, 8, torch.Generator().manual_seed(1)))
    s, a, r, s1, gamma = b
    r = r.reshape(-1).contiguous()
    out = torch.empty(4, device="cuda")

    def call(eng):
        rc = lib.sfx_tsf_phi_update(eng.handle, 0, s.data_ptr(), a.data_ptr(), r.data_ptr(), s1.data_ptr(),
                                    gamma.data_ptr(), 8, 1, eng.test_wb.data_ptr(), eng.test_lam.data_ptr(),
                                    out.data_ptr(), None)
        return rc, lib.sfx_last_error().decode()

    eng = engine_of(st, 3, tsf=False, phi=None)
    eng.tsf_setup(net.d, 0)
    rc, msg = call(eng)
    assert rc == -1 and "sfx_phi_setup" in msg, (rc, msg)
    eng.close()
    eng = engine_of(st, 3, tsf=False)
    rc, msg = call(eng)
    assert rc == -1 and "sfx_tsf_setup" in msg, (rc, msg)
    for G, K in ((net.d + 4, 0), (net.d, 2)):
        eng.tsf_setup(G, K)
        rc, msg = call(eng)
        assert rc == -1 and "G = d and K = 0" in msg, (G, K, rc, msg)
    # the wide setup's own limits; sfx_phi_setup keeps its limit and its text
    assert lib.sfx_phi_setup_dims(eng.handle, 2049, 3, ctypes.c_float(1e-3)) == -1
    assert lib.sfx_phi_setup_dims(eng.handle, 2048, 7, ctypes.c_float(1e-3)) == -1
    assert lib.sfx_phi_setup(eng.handle, 11, 3, ctypes.c_float(1e-3)) == -1
    assert "hidden <= 128" in lib.sfx_last_error().decode()
    eng.close()


def test_checkpoint_round_trip_wide(tmp_path):
    """A wide φ net, g and h round-trip through sfx.checkpoint; a continued update matches an
    uninterrupted one bit for bit (the reward-model biases and λ are the caller's tensors)."""
    from sfx import checkpoint

    net, T, B = TP.Net(6, 64, 9, 12, ("relu", "relu"), 200, 3), 3, 16
    st = problem(net, T, seed=8)
    eng = engine_of(st, 2)
    gen = torch.Generator().manual_seed(9)
    bs = [batch(net, B, gen) for _ in range(5)]
    for j in range(3):
        update(eng, j % T, bs[j], True)
    path = str(tmp_path / "sfx.pt")
    checkpoint.save(eng, path)
    other = problem(net, T, seed=10)  # other weights: everything must come from the file
    eng2 = engine_of(other, 2)
    checkpoint.load(eng2, path)
    eng2.test_wb.copy_(eng.test_wb)
    eng2.test_lam.copy_(eng.test_lam)
    assert eng2.phi_cfg == dict(hid=200, n_mid=3, lr=1e-3)
    for j in range(3, 5):
        l1, l2 = update(eng, j % T, bs[j], True).cpu(), update(eng2, j % T, bs[j], True).cpu()
        assert torch.equal(l1, l2), j
    a, b = gpu_state(eng, T), gpu_state(eng2, T)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    narrow = engine_of(problem(TP.Net(6, 64, 9, 12, ("relu", "relu"), 26, 3), T, seed=8), 2, phi="mul")
    with pytest.raises(ValueError, match="φ configuration"):
        checkpoint.load(narrow, path)
    for e in (eng, eng2, narrow):
        e.close()


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


def test_dropin_tsf_phi_vs_golden(golden, monkeypatch):
    """sfx.dropin's features.deep_tsf_phi.DeepSF_TSF_PHI under the reference's call convention: an agent
    with agents/tsfdqn_phi.py's attributes whose update_deep_models is bound by sfx.dropin.bind
    (update_deep_models(transitions, phi, i, loss_coefficient, use_gpi)) replays the gpi golden run --
    its losses, λ and the reward-model biases updated in place, after the sync the agent's φ net, g_i, h,
    ψ modules and fit_w as the reference left them, get_next_successors the target heads' output."""
    import types

    from sfx.dropin import _host, bind
    from sfx.dropin.features.deep import _flat, _unflat_into
    from sfx.dropin.features.deep_tsf_phi import DeepSF_TSF_PHI
    from tests.golden.recipe import agent_psi_lambda

    dev = torch.device("cuda", 0)
    monkeypatch.setattr(_host, "torch_device", lambda: dev)
    monkeypatch.setattr("sfx.dropin.features.deep.get_torch_device", lambda: dev)
    g = golden("upd_tsf_phi_gpi")
    st0 = TP.problem_of(g)
    net, T, k = st0.net, int(g["T"]), int(g["k"])
    sf = DeepSF_TSF_PHI(pytorch_model_handle=agent_psi_lambda(net.H, net.acts, 1e-3, dev), use_true_reward=False,
                        target_update_ev=int(g["target_update_ev"]))
    sf.reset()
    for t in range(T):
        sf.add_training_task(_Task(net.n_s, net.A, net.d, t))
    with torch.no_grad():
        for t in range(T):
            _unflat_into(sf.psi[t][0][0], st0.online[t])
            _unflat_into(sf.psi[t][1][0], st0.online[t])
            lin = list.__getitem__(sf.fit_w, t)
            assert lin.bias is not None and tuple(lin.weight.shape) == (1, net.d)
            lin.weight.copy_(st0.w[t].view(1, -1))
            lin.bias.copy_(st0.wb[t:t + 1])
    layers = []
    for j, (o, i) in enumerate(net.phi_dims):
        layers += [torch.nn.Linear(i, o)] + ([torch.nn.ReLU()] if j < len(net.phi_dims) - 1 else [])
    pm = torch.nn.Sequential(*layers).to(dev)
    _unflat_into(pm, st0.phi)

    class TSFDQN_PHI:  # the attributes of agents/tsfdqn_phi.py's agent that the binding reads
        def update_deep_models(self, *a):
            raise AssertionError("not bound")

        def test_agent(self, task, test_index):
            return "user test_agent"

    bind.patch("agents.tsfdqn_phi", types.SimpleNamespace(TSFDQN_PHI=TSFDQN_PHI))
    agent = TSFDQN_PHI()
    agent.sf = sf
    agent.phi = ((pm, torch.nn.MSELoss(), None), (None, None, None))
    agent.g_functions = [torch.nn.Linear(net.n_s, net.d).to(dev) for _ in range(T)]
    agent.h_function = torch.nn.Linear(net.d, net.d).to(dev)
    for t in range(T):
        _unflat_into(agent.g_functions[t], st0.g[t])
    _unflat_into(agent.h_function, st0.h)
    lams = [torch.ones(1, requires_grad=True, device=dev) for _ in range(T)]
    lam_ptrs = [x.data_ptr() for x in lams]
    for j, (s, a, r, s1, gamma) in enumerate(TP.batches_of(g)):
        i = int(g["policies"][j])
        agent.task_index, agent.g_function = i, agent.g_functions[i]
        b = tuple(x.to(dev) for x in (s, a, r, torch.empty(0), s1, gamma))
        with pytest.raises(NotImplementedError):
            agent.update_deep_models(b, agent.phi, (i + 1) % T, lams[i], True)
        loss, psi_loss, phi_loss, lam = agent.update_deep_models(b, agent.phi, i, lams[i], True)
        assert lam is lams[i]
        rel_close(torch.cat([loss, psi_loss, phi_loss, lam.detach()]).cpu(), g["losses"][j], rtol=1e-4, atol=1e-7)
    assert agent.update_deep_models(None, agent.phi, 0, lams[0], True) is None
    assert [x.data_ptr() for x in lams] == lam_ptrs
    rel_close(torch.cat([x.detach() for x in lams]).cpu(), g["lam"], rtol=1e-6, atol=1e-7)
    assert torch.equal(_flat(pm), st0.phi)  # the modules are stale until the sync
    assert agent.test_agent(None, 0) == "user test_agent"  # the agent's own method, after the sync
    params_close(_flat(pm), g["phi"], 1e-3 * k, max_bad_frac=2e-3)
    params_close(torch.stack([_flat(m) for m in agent.g_functions]), g["g"], 1e-3 * k, max_bad_frac=2e-3)
    params_close(_flat(agent.h_function), g["h"], 1e-3 * k, max_bad_frac=2e-3)
    params_close(torch.stack([_flat(sf.psi[t][0][0]) for t in range(T)]), g["online"], 1e-3 * k, max_bad_frac=2e-3)
    params_close(torch.stack([sf.fit_w[t].weight.detach().reshape(-1).cpu() for t in range(T)]), g["w"], 1e-3 * k)
    params_close(torch.stack([sf.fit_w[t].bias.detach().reshape(-1).cpu() for t in range(T)]).reshape(-1), g["wb"],
                 1e-3 * k)
    s = torch.from_numpy(g["b_s"][0][:4]).to(dev)
    nxt = sf.get_next_successors(s)
    assert nxt.shape == (4, T, net.A, net.d)
    want = torch.stack([TP.psi_forward(torch.from_numpy(g["target"][t]), net, s.cpu()) for t in range(T)], dim=1)
    rel_close(nxt.cpu(), want, rtol=1e-4, atol=1e-5)
    rel_close(sf.get_next_successor(s, 1).cpu(), want[:, 1], rtol=1e-4, atol=1e-5)
    q, task = sf.GPI_w(s, sf.fit_w[0])
    assert q.shape == (4, T, net.A) and task.shape == (4,)
    for fn in (lambda: sf.update_reward(None, None, 0), lambda: sf.update_successor(None, None, 0)):
        with pytest.raises(Exception, match="shouldn't be used"):
            fn()
