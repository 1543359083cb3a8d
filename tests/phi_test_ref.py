"""The learned-φ agents' test phase, restated with torch autograd: agents/tsfdqn_phi.py TSFDQN_PHI.get_test_action
(:381-397) and update_target_models (:434-505), agents/sfdqn_phi.py SFDQN_PHI.update_test_reward_mapper (:263-305).

    Ω = agent.omegas = Linear(T d, d) (shared by the test tasks), w = the test task's Linear(d, 1) with bias,
    flat(ψ)[a] = concat_t ψ_t[a]                                  (swapaxes(1, 2).flatten(start_dim=2))
    action:  argmax_a w(Ω(flat(ψ(s))[a]))
    update:  φ̃ = φ_net(s ⊕ a ⊕ s1) ⊙ (h(Ω(concat_t g_t(s))) + h(Ω(concat_t g_t(s1))))
             psi_loss = MSE(Ω(flat(ψ(s))), φ̃ + γ Ω(flat(ψ⁻(s1)))), phi_loss = MSE(w(φ̃), r)
             loss = phi_loss + λ psi_loss; gradients clamped to ±1e10, one step of a freshly built Adam (lr 1e-3):
             descent on w, b_w, Ω, ascent on λ; λ clamped to [1e-2, 1e6].  ψ, ψ⁻, g, h, the φ net: not trained.
    SF-φ:    loss = MSE(w(φ_net(s ⊕ a ⊕ s1)), r), one fresh Adam step on w, b_w.

Generic in dtype and device (the tensors decide), built on tests/tsf_phi_ref.py's State (heads, φ net, g, h) and
pinned against the real reference by tests/test_phi_test_golden.py over tests/golden/test_{tsf_phi,phi}.npz.
``action=`` replaces the greedy action, so a float64 run can follow an fp32 run's actions.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F

from tests import tsf_phi_ref as TP


@dataclass
class TestTask:
    """A test task's trainable state; omega_w / omega_b are the AGENT's Ω (every test task updates it)."""
    omega_w: torch.Tensor   # [d, T d]
    omega_b: torch.Tensor   # [d]
    w: torch.Tensor         # [d]   Linear(d, 1).weight
    wb: torch.Tensor        # [1]   Linear(d, 1).bias
    lam: torch.Tensor       # [1]   the test task's loss coefficient

    __test__ = False  # not a pytest class

    def to(self, dtype=None, device=None):
        f = lambda x: x.detach().clone().to(dtype=dtype, device=device)
        return TestTask(f(self.omega_w), f(self.omega_b), f(self.w), f(self.wb), f(self.lam))

    def groups(self):
        return dict(omega_w=self.omega_w, omega_b=self.omega_b, w=self.w, wb=self.wb, lam=self.lam)


def flat_psi(heads, net: TP.Net, s):
    """flat(ψ(s)): [A, T d] from the packed heads [T, P_psi] and one state [n_s]."""
    psi = torch.stack([TP.psi_forward(heads[t], net, s.reshape(1, -1))[0] for t in range(heads.shape[0])])  # [T, A, d]
    return psi.swapaxes(0, 1).flatten(start_dim=1)


def q_values(st: TP.State, tt: TestTask, s):
    """q [A] of get_test_action's greedy branch."""
    with torch.no_grad():
        tp = F.linear(flat_psi(st.online, st.net, s), tt.omega_w, tt.omega_b)
        return F.linear(tp, tt.w.reshape(1, -1), tt.wb).reshape(-1)


def greedy(st: TP.State, tt: TestTask, s):
    """(action, top-2 gap of q, max |q|) -- the gap tells whether demanding the same action of another
    arithmetic is fair."""
    q = q_values(st, tt, s)
    top = torch.topk(q, 2).values
    return int(torch.argmax(q)), float(top[0] - top[1]), float(q.abs().max())


def sf_greedy(st: TP.State, tt: TestTask, s):
    """SFDQN_PHI.get_test_action's greedy branch (agents/sfdqn_phi.py:224-232): GPI_w with the test task's
    Linear(d, 1), q[t, a] = w(ψ_t(s)[a]); the action of the best task's row -> (a, gap of the table, max |q|)."""
    with torch.no_grad():
        psi = torch.stack([TP.psi_forward(st.online[t], st.net, s.reshape(1, -1))[0] for t in range(st.online.shape[0])])
        q = F.linear(psi, tt.w.reshape(1, -1), tt.wb)[..., 0]  # [T, A]
    c = int(torch.argmax(q.max(dim=1).values))
    top = torch.topk(q.reshape(-1), 2).values
    return int(torch.argmax(q[c])), float(top[0] - top[1]), float(q.abs().max())


def phi_of(st: TP.State, s, a, s1):
    inp = torch.cat([s.reshape(-1), torch.as_tensor(a, device=s.device).reshape(-1).to(s.dtype), s1.reshape(-1)])
    return TP.phi_forward(st.phi, st.net, inp.reshape(1, -1))[0]


def tsf_update(st: TP.State, tt: TestTask, s, a, r, s1, gamma: float, lr: float = 1e-3, as_tensors: bool = False,
               train_bias: bool = True):
    """One update_target_models(w, λ, r, s, a, s1) -> (loss, psi_loss, phi_loss); tt in place.
    train_bias=False: a reward model WITHOUT bias (tt.wb stays what it is, zero)."""
    net, T = st.net, st.online.shape[0]
    d, n_s = net.d, net.n_s
    s, s1 = s.reshape(-1), s1.reshape(-1)
    with torch.no_grad():
        phi = phi_of(st, s, a, s1)
        x = flat_psi(st.online, net, s)
        y = flat_psi(st.target, net, s1)
        c = torch.cat([TP.linear_flat(st.g[t], d, n_s, s) for t in range(T)])
        c1 = torch.cat([TP.linear_flat(st.g[t], d, n_s, s1) for t in range(T)])
    leaves = [tt.omega_w, tt.omega_b, tt.w, tt.wb, tt.lam]
    oW, ob, w, wb, lam = (p.detach().clone().requires_grad_(True) for p in leaves)
    aff = TP.linear_flat(st.h, d, d, F.linear(c, oW, ob)) + TP.linear_flat(st.h, d, d, F.linear(c1, oW, ob))
    tphi = phi * aff
    cur = F.linear(x, oW, ob)
    nxt = tphi + gamma * F.linear(y, oW, ob)
    phi_loss = F.mse_loss(F.linear(tphi, w.reshape(1, -1), wb), torch.as_tensor([r], dtype=s.dtype, device=s.device))
    psi_loss = F.mse_loss(cur, nxt)
    loss = phi_loss + lam * psi_loss
    loss.sum().backward()
    with torch.no_grad():
        for p, leaf in zip(leaves[:4], (oW, ob, w, wb)):
            if train_bias or p is not tt.wb:
                TP.fresh_adam_(p, leaf.grad.clamp(-1e10, 1e10), lr)
        TP.fresh_adam_(tt.lam, lam.grad.clamp(-1e10, 1e10), lr, maximize=True)
        tt.lam.clamp_(1e-2, 1e6)
    out = (loss.detach().reshape(()), psi_loss.detach(), phi_loss.detach())
    return out if as_tensors else tuple(float(v) for v in out)


def sf_update(st: TP.State, tt: TestTask, s, a, r, s1, lr: float = 1e-3, as_tensors: bool = False):
    """One update_test_reward_mapper(w, r, s, a, s1) -> loss; tt.w, tt.wb in place."""
    with torch.no_grad():
        phi = phi_of(st, s.reshape(-1), a, s1.reshape(-1))
    w, wb = (p.detach().clone().requires_grad_(True) for p in (tt.w, tt.wb))
    loss = F.mse_loss(F.linear(phi, w.reshape(1, -1), wb), torch.as_tensor([r], dtype=phi.dtype, device=phi.device))
    loss.backward()
    with torch.no_grad():
        TP.fresh_adam_(tt.w, w.grad.clamp(-1e10, 1e10), lr)
        TP.fresh_adam_(tt.wb, wb.grad.clamp(-1e10, 1e10), lr)
    return loss.detach() if as_tensors else float(loss.detach())


def tsf_step(st: TP.State, tt: TestTask, s, r, s1, gamma: float, action=None, lr: float = 1e-3):
    """One test step: the greedy action on s (``action`` replaces it), then the update on (s, a, r, s1).
    -> (a, gap, max |q|, (loss, psi_loss, phi_loss))."""
    a, gap, qmax = greedy(st, tt, s)
    if action is not None:
        a = int(action)
    return a, gap, qmax, tsf_update(st, tt, s, a, r, s1, gamma, lr)


# ---- fixtures of tools/gen_golden_phi_test.py ------------------------------------------------
def problem_of(g):
    """(State, TestTask) of a test_tsf_phi / test_phi fixture's initial state.  The SF-φ fixture has no g, h, Ω or
    λ: they come back as zeros / ones of the right shapes and sf_update never reads them."""
    net = TP.Net(int(g["n_s"]), int(g["H"]), int(g["A"]), int(g["d"]), tuple(str(a) for a in g["acts"]),
                 int(g["hid"]), int(g["n_mid"]))
    T, d = int(g["T"]), net.d
    t = lambda k, alt: torch.from_numpy(g[k]).clone() if k in g else alt
    st = TP.State(net, t("online", None), t("target", None), torch.zeros(T, d), torch.zeros(T), t("phi", None),
                  t("g", torch.zeros(T, d * net.n_s + d)), t("h", torch.zeros(d * d + d)), torch.ones(T))
    tt = TestTask(t("omega_w0", torch.zeros(d, T * d)), t("omega_b0", torch.zeros(d)), t("w0", None), t("wb0", None),
                  t("lam0", torch.ones(1)))
    return st, tt


def final_of(g, tt0: TestTask) -> TestTask:
    t = lambda k, alt: torch.from_numpy(g[k]).clone() if k in g else alt.clone()
    return TestTask(t("omega_w", tt0.omega_w), t("omega_b", tt0.omega_b), t("w", tt0.w), t("wb", tt0.wb),
                    t("lam", tt0.lam))


def steps_of(g):
    """[(s, a, r, s1)] of the recorded chain."""
    return [(torch.from_numpy(g["s"][j]), int(g["a"][j]), float(g["r"][j]), torch.from_numpy(g["s1"][j]))
            for j in range(int(g["k"]))]
