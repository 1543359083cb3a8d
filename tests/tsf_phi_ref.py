"""TSF-DQN with a learned φ, restated with torch autograd: agents/tsfdqn_phi.py
TSFDQN_PHI.update_deep_models (:180-288) over features/deep_tsf_phi.py DeepSF_TSF_PHI, and (with
``transform=False``) features/deep_phi.py DeepSF_PHI.update_successor for a φ net of any hidden width.

    φ̃ = φ_net(s ⊕ a ⊕ s1) ⊙ (h(g_i(s)) + h(g_i(s1))),  g_i = Linear(n_s, d), h = Linear(d, d)
    targets = φ̃ + γ ψ⁻_i(s1)[a'] (they carry φ̃'s gradient), loss = MSE(w_i(φ̃), r) + λ_i MSE(ψ_i(s), merged)
    gradients clamped to [-1, 1], one step of a freshly built Adam (lr 1e-3) on ψ_i, φ, g_i, h, w_i, b_i,
    ascent on λ_i, λ_i clamped to [1e-2, 1e6]; target sync every target_update_ev updates of a policy.

Generic in dtype and device (the state's tensors decide), self-contained (pinned against the real
reference by tests/test_tsf_phi_golden.py over tests/golden/upd_tsf_phi_*.npz).  ``next_actions``
replaces the argmax, so a float64 run can follow an fp32 run's actions.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

import torch
import torch.nn.functional as F


@dataclass
class Net:
    n_s: int
    H: int
    A: int
    d: int
    acts: Tuple[str, ...]   # ψ head: Linear(n_s, H), (Linear(H, H) + act) per entry, Linear(H, A d)
    hid: int                # φ net: Linear(2 n_s + 1, hid) + ReLU, n_mid × (Linear(hid, hid) + ReLU), Linear(hid, d)
    n_mid: int = 3

    @property
    def psi_dims(self) -> List[Tuple[int, int]]:
        return [(self.H, self.n_s)] + [(self.H, self.H)] * len(self.acts) + [(self.A * self.d, self.H)]

    @property
    def phi_dims(self) -> List[Tuple[int, int]]:
        n_in = 2 * self.n_s + 1
        return [(self.hid, n_in)] + [(self.hid, self.hid)] * self.n_mid + [(self.d, self.hid)]

    @property
    def P_psi(self) -> int:
        return sum(o * i + o for o, i in self.psi_dims)

    @property
    def P_phi(self) -> int:
        return sum(o * i + o for o, i in self.phi_dims)


def _unpack(flat, dims):
    out, off = [], 0
    for o, i in dims:
        out.append((flat[off:off + o * i].view(o, i), flat[off + o * i:off + o * i + o]))
        off += o * i + o
    return out


def psi_forward(flat, net: Net, X):
    """ψ(X) of one head: [B, A, d]."""
    acts = (None,) + tuple(net.acts) + (None,)
    y = X
    for (W, b), a in zip(_unpack(flat, net.psi_dims), acts):
        y = F.linear(y, W, b)
        y = torch.relu(y) if a == "relu" else torch.tanh(y) if a == "tanh" else y
    return y.view(X.shape[0], net.A, net.d)


def phi_forward(flat, net: Net, X):
    layers = _unpack(flat, net.phi_dims)
    y = X
    for l, (W, b) in enumerate(layers):
        y = F.linear(y, W, b)
        if l < len(layers) - 1:
            y = torch.relu(y)
    return y


def linear_flat(flat, n_out, n_in, X):
    """A Linear(n_in, n_out) packed W [out][in], b [out]."""
    return F.linear(X, flat[:n_out * n_in].view(n_out, n_in), flat[n_out * n_in:n_out * n_in + n_out])


@dataclass
class State:
    net: Net
    online: torch.Tensor   # [T, P_psi]
    target: torch.Tensor   # [T, P_psi]
    w: torch.Tensor        # [T, d]   Linear(d, 1).weight rows
    wb: torch.Tensor       # [T]      Linear(d, 1).bias
    phi: torch.Tensor      # [P_phi]  the shared φ net
    g: torch.Tensor        # [T, d n_s + d]  g_i
    h: torch.Tensor        # [d d + d]       the shared h
    lam: torch.Tensor      # [T]      the agent's loss coefficients
    since_target: List[int] = field(default_factory=list)

    def __post_init__(self):
        if not self.since_target:
            self.since_target = [0] * self.online.shape[0]

    def to(self, dtype=None, device=None):
        f = lambda x: x.detach().clone().to(dtype=dtype, device=device)
        return State(self.net, f(self.online), f(self.target), f(self.w), f(self.wb), f(self.phi), f(self.g),
                     f(self.h), f(self.lam), list(self.since_target))


def fresh_adam_(p, g, lr, maximize=False, betas=(0.9, 0.999), eps=1e-8):
    """One step of a freshly built torch Adam (moments zero, step 1), torch/optim/adam.py's arithmetic."""
    g = -g if maximize else g
    m = torch.zeros_like(p).lerp_(g, 1 - betas[0])
    v = torch.zeros_like(p).addcmul_(g, g, value=1 - betas[1])
    denom = (v.sqrt() / ((1 - betas[1]) ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / (1 - betas[0])))


def update(st: State, batch, i: int, *, use_gpi: bool = True, lr: float = 1e-3, target_update_ev: int = 1000,
           next_actions=None, transform: bool = True, as_tensors: bool = False):
    """One update_deep_models(transitions, phi, i, λ_i, use_gpi) (transform=False: DeepSF_PHI's
    update_successor, no g / h and no clamp) -> (loss, psi_loss, phi_loss, λ_i, next actions); st in place.
    as_tensors: the four values as tensors on the state's device, no host read (timing on a GPU)."""
    s, a, r, s1, gamma = batch
    net = st.net
    B, d, n_s, T = s.shape[0], net.d, net.n_s, st.online.shape[0]
    idx = torch.arange(B, device=s.device)
    gamma = gamma.reshape(-1, 1)
    with torch.no_grad():
        heads = range(T) if use_gpi else [i]
        psi1 = torch.stack([psi_forward(st.online[t], net, s1) for t in heads], dim=1)   # [B, T', A, d]
        q1 = torch.matmul(psi1, st.w[i].reshape(-1, 1))[..., 0] + st.wb[i]
        nxt = torch.argmax(torch.max(q1, dim=1).values, dim=-1)
        if next_actions is not None:
            nxt = torch.as_tensor(next_actions, device=s.device)
        tpsi = psi_forward(st.target[i], net, s1)
    leaves = [st.online[i], st.phi, st.w[i], st.wb[i].reshape(1), st.lam[i].reshape(1), st.g[i], st.h]
    pt, ph, w, wb, lam, gi, hh = (x.detach().clone().requires_grad_(True) for x in leaves)
    inp = torch.cat([s, a.reshape(B, 1).to(s.dtype), s1], dim=1)
    phis = phi_forward(ph, net, inp)
    if transform:
        phis = phis * (linear_flat(hh, d, d, linear_flat(gi, d, n_s, s)) + linear_flat(hh, d, d, linear_flat(gi, d, n_s, s1)))
    cur = psi_forward(pt, net, s)
    targets = phis + gamma * tpsi[idx, nxt, :]
    merged = cur.clone()
    merged[idx, a, :] = targets
    phi_loss = F.mse_loss(F.linear(phis, w.reshape(1, -1), wb), r.reshape(B, 1))
    psi_loss = F.mse_loss(cur, merged)
    loss = phi_loss + lam * psi_loss
    loss.backward()
    with torch.no_grad():
        trained = [(st.online[i], pt), (st.phi, ph), (st.w[i], w), (st.wb[i:i + 1], wb)]
        if transform:
            trained += [(st.g[i], gi), (st.h, hh)]
        for p, leaf in trained:
            fresh_adam_(p, leaf.grad.clamp(-1, 1) if transform else leaf.grad, lr)
        fresh_adam_(st.lam[i:i + 1], lam.grad.clamp(-1, 1) if transform else lam.grad, lr, maximize=True)
        st.lam[i:i + 1].clamp_(1e-2, 1e6)
    st.since_target[i] += 1
    if st.since_target[i] >= target_update_ev:
        st.target[i].copy_(st.online[i])
        st.since_target[i] = 0
    if as_tensors:
        return loss.detach(), psi_loss.detach(), phi_loss.detach(), st.lam[i], nxt
    return float(loss.detach()), float(psi_loss.detach()), float(phi_loss.detach()), float(st.lam[i]), nxt


def problem_of(g, hid=None) -> State:
    """The initial state of an upd_tsf_phi_* fixture (tools/gen_golden_tsf_phi.py)."""
    net = Net(int(g["n_s"]), int(g["H"]), int(g["A"]), int(g["d"]), tuple(str(a) for a in g["acts"]),
              int(g["hid"]), int(g["n_mid"]))
    T = int(g["T"])
    t = lambda k: torch.from_numpy(g[k]).clone()
    return State(net, t("online0"), t("online0"), t("w0"), t("wb0"), t("phi0"), t("g0"), t("h0"), torch.ones(T))


def final_of(g, st0: State) -> State:
    t = lambda k: torch.from_numpy(g[k]).clone()
    return State(st0.net, t("online"), t("target"), t("w"), t("wb"), t("phi"), t("g"), t("h"), t("lam").float())


def batches_of(g):
    return [tuple(torch.from_numpy(g[f"b_{n}"][j]) for n in ("s", "a", "r", "s1", "gamma")) for j in range(int(g["k"]))]
