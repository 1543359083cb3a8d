"""Gradient VALUES of every update path, for tests/test_grad_ref.py (CPU) and tests/test_gpu_gradients.py.

Adam hides the size of a gradient: a persistent Adam's parameters move by m̂/√v̂ and a freshly built one's by
lr·g/(|g| + 1e-8) = ±lr, so a parameter comparison sees signs only.  This module has

  * autograd oracles of every update's loss, generic in dtype (float64: the reference; float32: the reference's
    own rounding error), that return one gradient per parameter group in the engine's packing and follow given
    next actions.  They share nothing with the manual backward of oracle/ref_cpu.py (forward passes only);
  * the two ways a gradient is read back through the library's ABI:
      1. first-step moments: from zero moments m = (1-β1) g, v = (1-β2) g²; a second consecutive step gives
         g₂ = (m₂ - β1 m₁)/(1-β1) (grad_from_moments);
      2. a fresh-Adam step with ε = lr = 1: Δp = -g/(|g| + 1), so g = -Δ/(1 - |Δ|) (grad_from_step);
  * grad_close, the comparison: every element, max |got - ref64| <= max(4 · max |ref32 - ref64|, 1e-5 · max |ref64|)
    per group, ref32 being the float32 oracle pushed through the same recovery.  1e-5 is about 5x the worst
    float32-oracle error measured over the test shapes and 270x below the smallest wrong-gradient mutation measured
    (one of 32 batch rows dropped from a bias sum: 2.7e-3); the factor 4 on the reference's own error follows the
    error-budget tests, which bound the GPU by a small multiple of the fp32 reference's error plus a floor
    (tests/test_gpu_phi.py);
  * the cases (shapes, seeds) both test files run, and their problems.  The inputs stay away from the kinks where
    float32 and float64 gradients differ discretely (Info.check): ReLU biases are nudged off the rows' zero
    crossings (clear_kinks), and a case's seed is the first for which the other conditions hold; `python -m
    tests.grad_ref` searches the seeds again.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from tests import phi_test_ref as PT
from tests import tsf_phi_ref as TP

B1, B2 = 0.9, 0.999
F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------
# recovery
# ---------------------------------------------------------------------------------------------
def grad_from_moments(m, m_prev=None) -> torch.Tensor:
    """Recipe 1: the gradient of the step that left first moment m (m_prev: the moment before it, zero if None)."""
    m = torch.as_tensor(m).detach().cpu().double()
    if m_prev is not None:
        m = m - B1 * torch.as_tensor(m_prev).detach().cpu().double()
    return m / (1 - B1)


def second_moment_of(g, v_prev=None) -> torch.Tensor:
    """v after a step with gradient g (from v_prev, zero if None)."""
    v = (1 - B2) * torch.as_tensor(g).double() ** 2
    return v if v_prev is None else v + B2 * torch.as_tensor(v_prev).detach().cpu().double()


def grad_from_step(before, after, ascent: bool = False) -> torch.Tensor:
    """Recipe 2: the gradient behind one fresh-Adam step with ε = lr = 1 (ascent: a maximised parameter)."""
    d = torch.as_tensor(after).detach().cpu().double() - torch.as_tensor(before).detach().cpu().double()
    g = -d / (1 - d.abs())
    return -g if ascent else g


def fresh_step(p: torch.Tensor, g: torch.Tensor, ascent: bool = False) -> torch.Tensor:
    """p after recipe 2's step, in p's dtype (tests/tsf_phi_ref.py's fresh Adam at ε = lr = 1)."""
    q = p.detach().clone()
    TP.fresh_adam_(q, g.to(q.dtype).reshape(q.shape), 1.0, maximize=ascent, eps=1.0)
    return q


def through_moments(g: torch.Tensor) -> torch.Tensor:
    """A float32 gradient through recipe 1 (what the float32 oracle's Adam would have stored)."""
    return grad_from_moments(torch.zeros_like(g).lerp_(g, 1 - B1))


def through_step(p: torch.Tensor, g: torch.Tensor, ascent: bool = False) -> torch.Tensor:
    """A float32 gradient through recipe 2 on the float32 parameter p."""
    return grad_from_step(p, fresh_step(p, g, ascent), ascent)


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
FLOOR = 1e-5
ROWS: List[Tuple[str, float, float, float, float]] = []   # (group, GPU error, fp32-reference error, max |g|, bound)


def grad_bound(ref64, ref32=None, floor: float = FLOOR) -> Tuple[float, float, float]:
    """(bound, fp32-reference error, max |ref64|) of one group."""
    ref64 = torch.as_tensor(ref64).detach().cpu().double().reshape(-1)
    scale = float(ref64.abs().max())
    e32 = 0.0 if ref32 is None else float((torch.as_tensor(ref32).detach().cpu().double().reshape(-1) - ref64).abs().max())
    return max(4.0 * e32, floor * scale), e32, scale


def grad_close(name: str, got, ref64, ref32=None, floor: float = FLOOR) -> float:
    """Every element of `got` within the bound of the float64 gradient; prints one row and returns the error.
    floor: the relative floor, 1e-5 unless a group's row in profiles/gradient_error.md justifies more (<= 1e-4)."""
    assert floor <= 1e-4
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref64).detach().cpu().double().reshape(-1)
    assert got.numel() == ref.numel(), f"{name}: {got.numel()} elements, the oracle has {ref.numel()}"
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite gradient"
    bound, e32, scale = grad_bound(ref, ref32, floor)
    assert scale > 0, f"{name}: the oracle's gradient is identically zero"
    err = float((got - ref).abs().max())
    ROWS.append((name, err, e32, scale, bound))
    print(f"| {name} | {err:.2e} | {e32:.2e} | {scale:.2e} | {bound:.2e} |")
    assert err <= bound, f"{name}: max |got - ref64| = {err:.3e} > {bound:.3e} (fp32 reference {e32:.3e}, max |g| {scale:.3e})"
    return err


def params_check(p, got, ref64, lr: float = 1e-3, frac: float = 2e-3) -> bool:
    """What the parameter comparisons see of a gradient: the parameters after a freshly built Adam's step
    (ε = 1e-8) with `got` against those with ref64, by the rule of tests/test_gpu_engine.py params_close with the
    learned-φ tests' excused fraction."""
    a, b = p.detach().double().clone().reshape(-1), p.detach().double().clone().reshape(-1)
    TP.fresh_adam_(a, torch.as_tensor(got).double().reshape(-1), lr)
    TP.fresh_adam_(b, torch.as_tensor(ref64).double().reshape(-1), lr)
    bad = (a - b).abs() > 1e-5 + 1e-4 * b.abs()
    return float(bad.double().mean()) <= frac and (not bool(bad.any()) or float((a - b).abs()[bad].max()) <= 2 * lr + 1e-5)


# ---------------------------------------------------------------------------------------------
# input conditions
# ---------------------------------------------------------------------------------------------
@dataclass
class Info:
    """What an oracle saw on the way: the next actions it followed and the distances from the kinks."""
    next: torch.Tensor
    q_gap: float = math.inf      # smallest top-2 gap of the next-action values / max |q|
    relu_min: float = math.inf   # smallest |pre-activation| of a differentiated ReLU
    td_min: float = math.inf     # smallest |TD error|
    kink_min: float = math.inf   # smallest relative distance of a Huber / clamped gradient from δ / the bound
    clamped: Dict[str, int] = field(default_factory=dict)   # entries beyond the clamp, per group
    psi_max: float = 0.0         # max |g_ψ| (the ψ epilogue leaves the clamp out)

    def check(self, what: str = "", relu: float = 1e-4, kink: float = 1e-4, gap: float = 1e-4):
        assert self.relu_min > relu, f"{what}: a ReLU pre-activation at {self.relu_min:.2e}"
        assert self.kink_min > kink, f"{what}: a gradient {self.kink_min:.2e} (relative) from its kink"
        assert self.td_min > 0, f"{what}: a TD error is exactly 0"
        assert self.q_gap >= gap, f"{what}: next-action top-2 gap {self.q_gap:.2e} of max |q|"

    def ok(self) -> bool:
        try:
            self.check()
        except AssertionError:
            return False
        return True


def cast(x, dtype):
    """Deep copy with every floating tensor in dtype."""
    if isinstance(x, dict):
        return {k: cast(v, dtype) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return type(x)(cast(v, dtype) for v in x)
    if torch.is_tensor(x):
        return x.detach().clone().to(dtype) if x.is_floating_point() else x.clone()
    if hasattr(x, "to") and hasattr(x, "__dataclass_fields__"):
        return x.to(dtype=dtype)
    return x


def _leaf(x):
    return x.detach().clone().requires_grad_(True)


# ---------------------------------------------------------------------------------------------
# networks (forward only; autograd does the rest)
# ---------------------------------------------------------------------------------------------
def mlp(flat, dims, acts, X, pre: Optional[list] = None, linear=F.linear):
    """Packed Linears (W [out][in], b [out]) with `acts` after each; ReLU pre-activations appended to pre.
    linear: the Linear itself, called once per layer in order (tests/bf16_ref.py: the bf16 operand emulation)."""
    y, off = X, 0
    for (o, i), a in zip(dims, acts):
        y = linear(y, flat[off:off + o * i].view(o, i), flat[off + o * i:off + o * i + o])
        off += o * i + o
        if a == "relu":
            if pre is not None:
                pre.append(y.detach())
            y = torch.relu(y)
        elif a == "tanh":
            y = torch.tanh(y)
    return y


def _psi_layout(spec):
    dims = [(spec.H, spec.n_s)] + [(spec.H, spec.H)] * len(spec.acts) + [(spec.A * spec.d, spec.H)]
    return dims, (None,) + tuple(spec.acts) + (None,)


def psi(flat, spec, X, pre=None, linear=F.linear):
    """ψ(X) of one head [B, A, d]; spec: anything with n_s, H, A, d, acts (oracle Spec, tsf_phi_ref Net)."""
    return mlp(flat, *_psi_layout(spec), X, pre, linear).view(X.shape[0], spec.A, spec.d)


def _phi_layout(net: TP.Net):
    return net.phi_dims, ("relu",) * (len(net.phi_dims) - 1) + (None,)


def phi_net(flat, net: TP.Net, X, pre=None):
    return mlp(flat, *_phi_layout(net), X, pre)


MARGIN = 1e-3


def clear_kinks(flat, dims, acts, X, margin: float = MARGIN):
    """Make a problem whose ReLUs stay away from zero on the rows X: the bias of every ReLU unit with a
    pre-activation inside ±margin moves (in place, layer by layer) by the smallest multiple of the margin that
    takes all of the unit's pre-activations out of it.  With tens of thousands of pre-activations per update no
    seed alone keeps every one of them 1e-4 away from the kink; a handful of biases moved by ~1e-3 does."""
    with torch.no_grad():
        y, off = X, 0
        for (o, i), a in zip(dims, acts):
            b = flat[off + o * i:off + o * i + o]
            z = F.linear(y, flat[off:off + o * i].view(o, i), b)
            off += o * i + o
            if a == "relu":
                for j in (z.abs().min(dim=0).values < margin).nonzero().flatten().tolist():
                    k, step = 1, None
                    while step is None:
                        step = next((t for t in (k * margin, -k * margin) if float((z[:, j] + t).abs().min()) >= margin),
                                    None)
                        k += 1
                    b[j] += step
                    z[:, j] += step
                y = torch.relu(z)
            else:
                y = torch.tanh(z) if a == "tanh" else z
    return flat


def next_actions_of(online, w_i, wb, spec, s1, i: int, use_gpi: bool, make_linear=None):
    """argmax_a max_t (ψ_t(s1)[a]·w_i + b) over all heads (GPI) or head i -> (actions [B], top-2 gap / max |q|)."""
    heads = range(online.shape[0]) if use_gpi else [i]
    lin = make_linear or (lambda: F.linear)
    psi1 = torch.stack([psi(online[t], spec, s1, linear=lin()) for t in heads], dim=1)
    q = torch.matmul(psi1, w_i.reshape(-1, 1))[..., 0] + wb
    x = q.max(dim=1).values
    top = torch.topk(x, 2, dim=1).values
    return torch.argmax(x, dim=-1), float((top[:, 0] - top[:, 1]).min() / q.abs().max())


def td_loss(cur, a, targets, huber: float = 0.0):
    """MSE (Huber) of ψ(s) against itself with the taken action's row replaced by the targets."""
    merged = cur.clone()
    merged[torch.arange(cur.shape[0]), a, :] = targets
    return F.huber_loss(cur, merged, delta=huber) if huber > 0 else F.mse_loss(cur, merged)


def _info(nxt, gap, pre, td, huber=0.0) -> Info:
    info = Info(nxt, gap)
    if pre:
        info.relu_min = min(float(z.abs().min()) for z in pre)
    info.td_min = float(td.abs().min())
    if huber > 0:
        info.kink_min = float(((td.abs() - huber).abs() / huber).min())
    return info


# ---------------------------------------------------------------------------------------------
# ψ paths: sfx_update, and one head of the all-task step
# ---------------------------------------------------------------------------------------------
def sf_grads(st, spec, batch, i: int, use_gpi: bool = True, huber: float = 0.0, next_actions=None, make_linear=None):
    """DeepSF.update_successor: l1 (+ l2 = MSE(w_i·φ, r) when r is given).  st: dict(online, target, w);
    batch = (s, a, r or None, φ, s1, γ) -> ({psi, [w]}, Info).  make_linear: called once per network forward
    for its `linear=` argument (None: F.linear)."""
    s, a, r, phi, s1, gamma = batch
    B = s.shape[0]
    idx = torch.arange(B)
    lin = make_linear or (lambda: F.linear)
    with torch.no_grad():
        nxt, gap = next_actions_of(st["online"], st["w"][i], 0.0, spec, s1, i, use_gpi, make_linear)
        if next_actions is not None:
            nxt = torch.as_tensor(next_actions)
        targets = phi + gamma.reshape(-1, 1) * psi(st["target"][i], spec, s1, linear=lin())[idx, nxt, :]
    pt, wi = _leaf(st["online"][i]), _leaf(st["w"][i])
    pre = []
    cur = psi(pt, spec, s, pre, linear=lin())
    loss = td_loss(cur, a, targets, huber)
    if r is not None:
        loss = loss + F.mse_loss(F.linear(phi, wi.reshape(1, -1)), r.reshape(B, 1))
    loss.backward()
    grads = {"psi": pt.grad}
    if r is not None:
        grads["w"] = wi.grad
    return grads, _info(nxt, gap, pre, (cur[idx, a, :] - targets).detach(), huber)


def adam_(p, g, m, v, step: int, lr: float, eps: float, betas=(B1, B2), wd: float = 0.0):
    R.adam_(p, g, m, v, step, lr, betas=betas, eps=eps, weight_decay=wd)


def all_task_step(st, mom, spec, batch, lr: float, eps: float, huber: float = 0.0, next_actions=None,
                  betas=(B1, B2), wd: float = 0.0):
    """The all-task step (every head on the same minibatch, in order, each GPI over the heads already updated;
    l1 only).  st["online"] and mom = dict(m, v [T, P], step [T]) advance -> [(grads, Info)] per head."""
    s, a, phi, s1, gamma = batch
    out = []
    for i in range(st["online"].shape[0]):
        g, info = sf_grads(st, spec, (s, a, None, phi, s1, gamma), i, True, huber,
                           None if next_actions is None else next_actions[i])
        mom["step"][i] += 1
        adam_(st["online"][i], g["psi"], mom["m"][i], mom["v"][i], mom["step"][i], lr, eps, betas, wd)
        out.append((g, info))
    return out


def zero_moments(x):
    return dict(m=torch.zeros_like(x), v=torch.zeros_like(x), step=[0] * x.shape[0])


# ---------------------------------------------------------------------------------------------
# TSF: sfx_tsf_update (ψ, w, g_i with K planar flows, h) and sfx_tsf_test_update (w, ω)
# ---------------------------------------------------------------------------------------------
def tsf_grads(st, spec, gs: R.GSpec, batch, i: int, use_gpi: bool, beta: float, next_actions=None):
    """TSFDQN.update_successor: φ̃ = (h(g_i(s)) + h(g_i(s1))) ⊙ φ in the targets and in l2; loss = l1 + β l2.
    st: dict(online, target, w, g [T, Pg], h) -> ({psi, w, g, h}, Info)."""
    s, a, r, phi, s1, gamma = batch
    B, d = s.shape[0], spec.d
    idx = torch.arange(B)
    with torch.no_grad():
        nxt, gap = next_actions_of(st["online"], st["w"][i], 0.0, spec, s1, i, use_gpi)
        if next_actions is not None:
            nxt = torch.as_tensor(next_actions)
        tpsi = psi(st["target"][i], spec, s1)[idx, nxt, :]
    pt, wi, gi, hh = (_leaf(x) for x in (st["online"][i], st["w"][i], st["g"][i], st["h"]))
    pre = []
    cur = psi(pt, spec, s, pre)
    Wh, bh = hh[:d * gs.G].view(d, gs.G), hh[d * gs.G:]
    tphi = (F.linear(R.g_forward(gi, gs, s)[0], Wh, bh) + F.linear(R.g_forward(gi, gs, s1)[0], Wh, bh)) * phi
    targets = tphi + gamma.reshape(-1, 1) * tpsi
    loss = td_loss(cur, a, targets) + beta * F.mse_loss(F.linear(tphi, wi.reshape(1, -1)), r.reshape(B, 1))
    loss.backward()
    return dict(psi=pt.grad, w=wi.grad, g=gi.grad, h=hh.grad), _info(nxt, gap, pre, (cur[idx, a, :] - targets).detach())


def tsf_test_grads(st, spec, gs: R.GSpec, w, omega, s, a: int, r: float, phi, s1, a1: int, gamma, beta, lasso):
    """TSFDQN.update_test_reward_mapper: loss = l1 + β l2 + lasso ||ω||_1 over w [d] and ω [T] -> {w, omega}."""
    d, T = spec.d, st["online"].shape[0]
    s, s1 = s.reshape(1, -1), s1.reshape(1, -1)
    with torch.no_grad():
        gs_s = torch.cat([R.g_forward(st["g"][t], gs, s)[0] for t in range(T)])
        gs_s1 = torch.cat([R.g_forward(st["g"][t], gs, s1)[0] for t in range(T)])
        p0 = torch.stack([psi(st["online"][t], spec, s)[0] for t in range(T)])
        p1 = torch.stack([psi(st["target"][t], spec, s1)[0] for t in range(T)])
    wl, om = _leaf(w), _leaf(omega)
    on = om / om.sum()
    Wh, bh = st["h"][:d * gs.G].view(d, gs.G), st["h"][d * gs.G:]
    tphi = phi.reshape(-1) * (F.linear((gs_s * on.view(-1, 1)).sum(0), Wh, bh)
                              + F.linear((gs_s1 * on.view(-1, 1)).sum(0), Wh, bh))
    nxt = tphi + gamma * (p1 * on.view(-1, 1, 1)).sum(0)[a1]
    cur = (p0 * on.view(-1, 1, 1)).sum(0)[a]
    loss = F.mse_loss(cur, nxt) + beta * ((tphi * wl).sum() - r) ** 2 + lasso * om.abs().sum()
    loss.backward()
    return dict(w=wl.grad, omega=om.grad)


# ---------------------------------------------------------------------------------------------
# learned φ: sfx_phi_update (transform=False), sfx_tsf_phi_update, and the test phase
# ---------------------------------------------------------------------------------------------
PHI_GROUPS = ("psi", "phi", "w", "wb", "lam")
TSF_PHI_GROUPS = PHI_GROUPS + ("g", "h")


def phi_grads(st: TP.State, batch, i: int, use_gpi: bool, transform: bool, next_actions=None):
    """DeepSF_PHI.update_successor / TSFDQN_PHI.update_deep_models: loss = MSE(w_i(φ̃), r) + λ_i MSE(ψ_i(s), merged),
    the targets carrying φ̃'s gradient; transform: φ̃ = φ ⊙ (h(g_i(s)) + h(g_i(s1))) and every gradient clamped to
    [-1, 1] -> ({psi, phi, w, wb, lam, [g, h]}, Info); λ's is the gradient of the loss (its step ascends)."""
    s, a, r, s1, gamma = batch
    net = st.net
    B, d, n_s = s.shape[0], net.d, net.n_s
    idx = torch.arange(B)
    with torch.no_grad():
        nxt, gap = next_actions_of(st.online, st.w[i], st.wb[i], net, s1, i, use_gpi)
        if next_actions is not None:
            nxt = torch.as_tensor(next_actions)
        tpsi = psi(st.target[i], net, s1)[idx, nxt, :]
    leaves = dict(psi=st.online[i], phi=st.phi, w=st.w[i], wb=st.wb[i].reshape(1), lam=st.lam[i].reshape(1))
    if transform:
        leaves.update(g=st.g[i], h=st.h)
    L = {k: _leaf(v) for k, v in leaves.items()}
    pre = []
    phis = phi_net(L["phi"], net, torch.cat([s, a.reshape(B, 1).to(s.dtype), s1], dim=1), pre)
    if transform:
        lin = TP.linear_flat
        phis = phis * (lin(L["h"], d, d, lin(L["g"], d, n_s, s)) + lin(L["h"], d, d, lin(L["g"], d, n_s, s1)))
    cur = psi(L["psi"], net, s, pre)
    targets = phis + gamma.reshape(-1, 1) * tpsi
    psi_loss = td_loss(cur, a, targets)
    loss = F.mse_loss(F.linear(phis, L["w"].reshape(1, -1), L["wb"]), r.reshape(B, 1)) + L["lam"] * psi_loss
    loss.backward()
    raw = {k: v.grad for k, v in L.items()}
    info = _info(nxt, gap, pre, (cur[idx, a, :] - targets).detach())
    info.psi_max = float(raw["psi"].abs().max())
    if not transform:
        return raw, info
    info.kink_min = min(float((v.abs() - 1).abs().min()) for v in raw.values())
    info.clamped = {k: int((v.abs() > 1).sum()) for k, v in raw.items()}
    return {k: v.clamp(-1, 1) for k, v in raw.items()}, info


def tsf_phi_test_grads(st: TP.State, tt: PT.TestTask, s, a: int, r: float, s1, gamma: float):
    """TSFDQN_PHI.update_target_models -> {omega_w, omega_b, w, wb, lam} (ψ, ψ⁻, g, h, the φ net not trained)."""
    net, T = st.net, st.online.shape[0]
    d, n_s = net.d, net.n_s
    s, s1 = s.reshape(-1), s1.reshape(-1)
    with torch.no_grad():
        phi = PT.phi_of(st, s, a, s1)
        x, y = PT.flat_psi(st.online, net, s), PT.flat_psi(st.target, net, s1)
        c = torch.cat([TP.linear_flat(st.g[t], d, n_s, s) for t in range(T)])
        c1 = torch.cat([TP.linear_flat(st.g[t], d, n_s, s1) for t in range(T)])
    L = {k: _leaf(v) for k, v in tt.groups().items()}
    om = lambda z: F.linear(z, L["omega_w"], L["omega_b"])
    tphi = phi * (TP.linear_flat(st.h, d, d, om(c)) + TP.linear_flat(st.h, d, d, om(c1)))
    phi_loss = F.mse_loss(F.linear(tphi, L["w"].reshape(1, -1), L["wb"]), torch.as_tensor([r], dtype=s.dtype))
    loss = phi_loss + L["lam"] * F.mse_loss(om(x), tphi + gamma * om(y))
    loss.sum().backward()
    return {k: v.grad for k, v in L.items()}


def phi_test_grads(st: TP.State, tt: PT.TestTask, s, a: int, r: float, s1):
    """SFDQN_PHI.update_test_reward_mapper: MSE(w(φ_net(s ⊕ a ⊕ s1)), r) -> {w, wb}."""
    with torch.no_grad():
        phi = PT.phi_of(st, s.reshape(-1), a, s1.reshape(-1))
    w, wb = _leaf(tt.w), _leaf(tt.wb)
    F.mse_loss(F.linear(phi, w.reshape(1, -1), wb), torch.as_tensor([r], dtype=phi.dtype)).backward()
    return dict(w=w.grad, wb=wb.grad)


# ---------------------------------------------------------------------------------------------
# cases and their problems (CPU; the GPU tests load the same tensors)
# ---------------------------------------------------------------------------------------------
LR_PSI, EPS_PSI = 1e-3, 1.0   # the ψ / TSF chains: ε = 1 keeps a step smooth in g (lr·g/(|g| + 1)), so the second
#                               step's parameters do not depend on the sign of a rounding-level gradient


@dataclass
class PsiCase:
    id: str
    shape: tuple            # (n_s, H, A, d, acts)
    B: int
    seed: int
    T: int = 3
    max_batch: int = 32
    single: bool = True     # sfx_update ±GPI too (False: the all-task step only)
    extras: bool = False    # sfx_step_all under forced re-runs and speculative rounds
    huber: bool = False     # also with HuberLoss(0.05)

    @property
    def spec(self):
        return R.Spec(*self.shape)


RR, R1, R3 = ("relu", "relu"), ("relu",), ("relu", "relu", "relu")
PSI_CASES = [
    PsiCase("ragged16", (17, 40, 7, 8, RR), 7, seed=0, extras=True, huber=True),   # ragged last 16-column layer-0 tile, half-valid dX sub-tile
    PsiCase("one_subtile", (4, 16, 7, 8, RR), 32, seed=0),   # a single sub-tile
    PsiCase("one_hidden", (17, 64, 7, 8, R1), 32, seed=0),   # one hidden layer, float4 rows
    PsiCase("one_row", (17, 64, 7, 8, RR), 1, seed=0),   # B = 1
    PsiCase("two_row_tiles", (17, 64, 7, 8, RR), 48, seed=0, max_batch=64),   # two row tiles, the unmerged launch sequence
    PsiCase("split_n_dx", (17, 512, 7, 8, RR), 8, seed=0, T=2),   # split-N dX
    PsiCase("many_heads", (17, 16, 7, 8, RR), 32, seed=7, T=40, single=False),   # T·A > 256: k_tdgw
    PsiCase("wide_fan_in", (70, 32, 3, 17, RR), 16, seed=0),   # fan-in past the fused layer-0 limit, odd d
    PsiCase("ad1350", (11, 48, 27, 50, RR), 45, seed=0, max_batch=64, huber=True),   # A·d = 1350: k_tdg
    PsiCase("tanh_three_tiles", (6, 40, 5, 3, ("tanh",)), 65, seed=0, max_batch=96),   # three row tiles, tanh
    PsiCase("three_hidden", (33, 96, 4, 12, R3), 33, seed=0, max_batch=64),   # three hidden layers, B one past a row tile
    PsiCase("c2", (17, 256, 7, 8, RR), 32, seed=2, T=8, extras=True),   # the flagship shape
]
HUBER = 0.05


def psi_problem(c: PsiCase):
    """(st = dict(online, target, w), [batch0, batch1]) with batch = (s, a, r, φ, s1, γ)."""
    from sfx.init import reference_heads

    spec = c.spec
    online, _ = reference_heads(c.T, spec.n_s, spec.H, spec.A, spec.d, spec.acts, seed=100 + c.seed)
    gen = torch.Generator().manual_seed(1000 + c.seed)
    u = lambda *shape, a: torch.empty(*shape).uniform_(-a, a, generator=gen)
    batches = [sf_batch(spec, c.B, gen) for _ in range(2)]
    for t in range(c.T):
        clear_kinks(online[t], *_psi_layout(spec), torch.cat([b[0] for b in batches]))
    st = dict(online=online, target=online + u(*online.shape, a=0.05), w=u(c.T, spec.d, a=0.5))
    return st, batches


def sf_batch(spec, B, gen):
    s, s1 = torch.randn(B, spec.n_s, generator=gen), torch.randn(B, spec.n_s, generator=gen)
    a = torch.randint(0, spec.A, (B,), generator=gen)
    phi, r = torch.rand(B, spec.d, generator=gen), torch.rand(B, 1, generator=gen)
    gamma = torch.where(torch.rand(B, generator=gen) < 0.1, 0.0, 0.9)
    return s, a, r, phi, s1, gamma


def psi_single_oracles(c: PsiCase, use_gpi: bool, huber: float = 0.0):
    """sfx_update of head T-1 on batch 0 from zero moments -> (ref64, ref32 through recipe 1, fp32 Info)."""
    st, (b, _) = psi_problem(c)
    g32, info = sf_grads(st, c.spec, b, c.T - 1, use_gpi, huber)
    g64, _ = sf_grads(cast(st, F64), c.spec, cast(b, F64), c.T - 1, use_gpi, huber, next_actions=info.next)
    return g64, {k: through_moments(v) for k, v in g32.items()}, info


def psi_all_oracles(c: PsiCase, huber: float = 0.0, steps: int = 2):
    """`steps` consecutive all-task steps (batch 0, then batch 1) from zero moments -> per step and head
    (ref64, ref32 through recipe 1, fp32 Info), and the float64 moments dict."""
    st, batches = psi_problem(c)
    s32, s64 = cast(st, F32), cast(st, F64)
    m32, m64 = zero_moments(s32["online"]), zero_moments(s64["online"])
    out = []
    for b in batches[:steps]:
        s, a, _, phi, s1, gamma = b
        prev = m32["m"].clone()
        r32 = all_task_step(s32, m32, c.spec, (s, a, phi, s1, gamma), LR_PSI, EPS_PSI, huber)
        r64 = all_task_step(s64, m64, c.spec, cast((s, a, phi, s1, gamma), F64), LR_PSI, EPS_PSI, huber,
                            next_actions=[info.next for _, info in r32])
        out.append([(g64["psi"], grad_from_moments(m32["m"][i], prev[i]), info)
                    for i, ((g64, _), (_, info)) in enumerate(zip(r64, r32))])
    return out, m64


# ---- TSF ------------------------------------------------------------------------------------
TSF_SHAPE, TSF_G, TSF_BETA, TSF_T = (11, 48, 5, 3, RR), 5, 0.5, 3
TSF_CASES = [(K, B, gpi) for K in (0, 2, 3, 4) for B in (7, 32) for gpi in (True, False)]
TSF_SEEDS: Dict[tuple, int] = {}   # by (K, B); 0 where not listed
TSF_TEST_HYPER = dict(gamma=0.9, beta=0.5, lasso=0.05)


def tsf_problem(K: int, B: int, seed: int):
    """(spec, gs, st = dict(online, target, w, g, h), [batch0, batch1], test = dict(w, omega, steps))."""
    from sfx.init import reference_heads

    spec, T = R.Spec(*TSF_SHAPE), TSF_T
    gs = R.GSpec(spec.n_s, TSF_G, K)
    online, _ = reference_heads(T, spec.n_s, spec.H, spec.A, spec.d, spec.acts, seed=200 + seed)
    gen = torch.Generator().manual_seed(2000 + seed)
    u = lambda *shape, a: torch.empty(*shape).uniform_(-a, a, generator=gen)
    batches = [sf_batch(spec, B, gen) for _ in range(2)]
    for t in range(T):
        clear_kinks(online[t], *_psi_layout(spec), torch.cat([b[0] for b in batches]))
    st = dict(online=online, target=online + u(*online.shape, a=0.05), w=u(T, spec.d, a=0.5), g=u(T, gs.P, a=0.3),
              h=u(spec.d * gs.G + spec.d, a=0.4))
    om = torch.rand(T, generator=gen) + 0.2
    steps = [(torch.randn(spec.n_s, generator=gen), int(torch.randint(0, spec.A, (1,), generator=gen)),
              float(torch.rand(1, generator=gen)), torch.rand(spec.d, generator=gen),
              torch.randn(spec.n_s, generator=gen), int(torch.randint(0, spec.A, (1,), generator=gen)))
             for _ in range(2)]
    return spec, gs, st, batches, dict(w=u(spec.d, a=0.5), omega=om / om.sum(), steps=steps)


TSF_GROUPS = ("psi", "w", "g", "h")
_TSF_KEYS = dict(psi="online", w="w", g="g", h="h")


def tsf_oracles(K: int, B: int, use_gpi: bool, seed: int, lr=None, wd=None, betas=(B1, B2), eps: float = EPS_PSI):
    """Two updates (policy 1 on batch 0, then policy 2 on batch 1) from zero moments -> per update
    (ref64, ref32 through recipe 1, fp32 Info); both of a policy's first step, so m = (1-β1) g.
    lr, wd: per group of TSF_GROUPS (LR_PSI and no decay where not given); the gradients are read with the
    default β1 whatever the step's betas."""
    lr, wd = lr or {}, wd or {}
    spec, gs, st, batches, _ = tsf_problem(K, B, seed)
    s32, s64 = cast(st, F32), cast(st, F64)
    out = []
    for i, b in zip((1, 2), batches):
        g32, info = tsf_grads(s32, spec, gs, b, i, use_gpi, TSF_BETA)
        g64, _ = tsf_grads(s64, spec, gs, cast(b, F64), i, use_gpi, TSF_BETA, next_actions=info.next)
        out.append((g64, {k: through_moments(v) for k, v in g32.items()}, info))
        for stx, g in ((s32, g32), (s64, g64)):   # the step itself: every policy's optimizer has its own moments
            for k in TSF_GROUPS:
                p = stx[_TSF_KEYS[k]] if k == "h" else stx[_TSF_KEYS[k]][i]
                adam_(p, g[k], torch.zeros_like(p), torch.zeros_like(p), 1, lr.get(k, LR_PSI), eps, betas, wd.get(k, 0.0))
    return out


def tsf_test_oracles(K: int, seed: int, wd_w: float = 0.0, wd_omega: float = 0.0):
    """sfx_tsf_test_update at step 1 and 2 (its own Adam state) -> per step (ref64, ref32 through recipe 1);
    wd_w, wd_omega: the decays of the two groups (they enter the moments the gradients are read from)."""
    spec, gs, st, _, test = tsf_problem(K, 7, seed)
    out = []
    tm = {}
    for dt in (F32, F64):
        stx, w, om = cast(st, dt), cast(test["w"], dt), cast(test["omega"], dt)
        mw, vw, mo, vo = (torch.zeros_like(x) for x in (w, w, om, om))
        res = []
        for k, (s, a, r, phi, s1, a1) in enumerate(test["steps"]):
            g = tsf_test_grads(stx, spec, gs, w, om, s.to(dt), a, r, phi.to(dt), s1.to(dt), a1, **TSF_TEST_HYPER)
            prev = (mw.clone(), mo.clone())
            adam_(w, g["w"], mw, vw, k + 1, LR_PSI, EPS_PSI, wd=wd_w)
            adam_(om, g["omega"], mo, vo, k + 1, LR_PSI, EPS_PSI, wd=wd_omega)
            om.clamp_(1e-7)
            res.append((g, dict(w=grad_from_moments(mw, prev[0]), omega=grad_from_moments(mo, prev[1]))))
        tm[dt] = res
    for (g64, _), (_, r32) in zip(tm[F64], tm[F32]):
        out.append((g64, r32))
    return out


# ---- learned φ -------------------------------------------------------------------------------
@dataclass
class PhiCase:
    hid: int
    B: int
    n_mid: int
    setup: str              # "dims" (sfx_phi_setup_dims) or "mul" (sfx_phi_setup)
    max_batch: int = 32
    d: int = 12
    reward_scale: float = 1.0
    seed: int = 0

    @property
    def id(self):
        return f"hid{self.hid}_B{self.B}_mid{self.n_mid}_{self.setup}_d{self.d}" + ("_x40" if self.reward_scale != 1 else "")

    @property
    def net(self):
        return TP.Net(6, 64, 9, self.d, RR, self.hid, self.n_mid)


PHI_T = 3
PHI_CASES = [PhiCase(8, 32, 3, "dims"), PhiCase(26, 32, 3, "mul"), PhiCase(128, 17, 1, "dims"),
             PhiCase(129, 17, 1, "dims"), PhiCase(131, 19, 3, "dims"), PhiCase(136, 7, 3, "dims"),
             PhiCase(200, 64, 3, "dims", max_batch=64), PhiCase(136, 48, 3, "dims", max_batch=64),
             PhiCase(136, 32, 3, "dims", d=3)]
CLAMP_CASE = PhiCase(136, 7, 3, "dims", reward_scale=40.0)
PHI_SEEDS: Dict[str, int] = {   # by PhiCase.id; 0 where not listed
    "hid8_B32_mid3_dims_d12": 1, "hid26_B32_mid3_mul_d12": 2, "hid128_B17_mid1_dims_d12": 1,
    "hid129_B17_mid1_dims_d12": 2, "hid131_B19_mid3_dims_d12": 1, "hid136_B7_mid3_dims_d12": 2,
    "hid136_B48_mid3_dims_d12": 2, "hid136_B32_mid3_dims_d3": 2, "hid136_B7_mid3_dims_d12_x40": 1}


def phi_problem(c: PhiCase, seed: int):
    """(TP.State with the targets moved off the online heads, batch = (s, a, r, s1, γ))."""
    from sfx.init import reference_heads

    net, T = c.net, PHI_T
    online, _ = reference_heads(T, net.n_s, net.H, net.A, net.d, net.acts, seed=300 + seed)
    gen = torch.Generator().manual_seed(3000 + seed)
    u = lambda *shape, a: torch.empty(*shape).uniform_(-a, a, generator=gen)
    target = online + u(*online.shape, a=0.05)
    target[:, -net.A * net.d:] += 1.0   # ψ⁻ one above ψ: TD errors of order 1, so that the ψ loss (λ's gradient)
    #                                     and λ ψ's gradient stand well above the rounding of a recipe-2 step
    st = TP.State(net, online, target, u(T, net.d, a=0.5), u(T, a=0.3), u(net.P_phi, a=0.15),
                  u(T, net.d * net.n_s + net.d, a=0.3), u(net.d * net.d + net.d, a=0.4),
                  torch.tensor([1.0, 4.0, 2.0])[:T].clone())
    B = c.B
    s, s1 = torch.randn(B, net.n_s, generator=gen), torch.randn(B, net.n_s, generator=gen)
    a = torch.randint(0, net.A, (B,), generator=gen)
    r = torch.rand(B, 1, generator=gen) * c.reward_scale
    gamma = torch.where(torch.rand(B, generator=gen) < 0.1, 0.0, 0.9)
    for t in range(T):
        clear_kinks(st.online[t], *_psi_layout(net), s)
    clear_kinks(st.phi, *_phi_layout(net), torch.cat([s, a.reshape(B, 1).float(), s1], dim=1))
    return st, (s, a, r, s1, gamma)


def phi_params(st: TP.State, i: int):
    """The parameter groups of policy i's update, by gradient name."""
    return dict(psi=st.online[i], phi=st.phi, w=st.w[i], wb=st.wb[i].reshape(1), lam=st.lam[i].reshape(1), g=st.g[i],
                h=st.h)


def phi_oracles(c: PhiCase, use_gpi: bool, transform: bool, seed: int, i: int = 1):
    """One update of policy i -> (ref64, ref32 through recipe 2 (ψ also through recipe 1 as "psi_m"), fp32 Info)."""
    st, b = phi_problem(c, seed)
    g32, info = phi_grads(st, b, i, use_gpi, transform)
    g64, _ = phi_grads(st.to(dtype=F64), cast(b, F64), i, use_gpi, transform, next_actions=info.next)
    p = phi_params(st, i)
    r32 = {k: through_step(p[k], v, ascent=k == "lam") for k, v in g32.items()}
    r32["psi_m"] = through_moments(g32["psi"])
    return g64, r32, info


# ---- learned φ: the test phase ---------------------------------------------------------------
PHI_TEST_CASES = [(hid, d) for hid in (26, 136) for d in (12, 3)]
PHI_TEST_SEEDS: Dict[tuple, int] = {}   # by (hid, d); 0 where not listed
GAMMA = 0.9


def phi_test_problem(hid: int, d: int, seed: int):
    """(TP.State, PT.TestTask, (s, a, r, s1)) at T = 3, A = 9."""
    c = PhiCase(hid, 1, 3, "mul" if hid == 26 else "dims", d=d)
    st, _ = phi_problem(c, 50 + seed)
    gen = torch.Generator().manual_seed(4000 + seed)
    u = lambda *shape, a: torch.empty(*shape).uniform_(-a, a, generator=gen)
    Td = PHI_T * d
    tt = PT.TestTask(u(d, Td, a=1 / math.sqrt(Td)), u(d, a=1 / math.sqrt(Td)), u(d, a=0.5), u(1, a=1 / math.sqrt(d)),
                     torch.ones(1))
    n_s = st.net.n_s
    step = (torch.randn(n_s, generator=gen), int(torch.randint(0, 9, (1,), generator=gen)),
            float(torch.rand(1, generator=gen)), torch.randn(n_s, generator=gen))
    return st, tt, step


def phi_test_oracles(hid: int, d: int, seed: int):
    """-> (tsf: (ref64, ref32 through recipe 2), sf: (ref64, ref32 through recipe 2))."""
    st, tt, (s, a, r, s1) = phi_test_problem(hid, d, seed)
    s64, t64 = st.to(dtype=F64), tt.to(dtype=F64)
    out = []
    for f, args32, args64 in ((tsf_phi_test_grads, (s, a, r, s1, GAMMA), (s.double(), a, r, s1.double(), GAMMA)),
                              (phi_test_grads, (s, a, r, s1), (s.double(), a, r, s1.double()))):
        g32, g64 = f(st, tt, *args32), f(s64, t64, *args64)
        p = tt.groups()
        out.append((g64, {k: through_step(p[k], v, ascent=k == "lam") for k, v in g32.items()}))
    return out


# ---------------------------------------------------------------------------------------------
# what each case compares: (label, {group: ref64}, {group: ref32 through the recovery}, Info or None)
# ---------------------------------------------------------------------------------------------
def psi_records(c: PsiCase):
    out = []
    for hub in (0.0, HUBER) if c.huber else (0.0,):
        tag = "huber " if hub else ""
        if c.single:
            for gpi in (True, False):
                g64, r32, info = psi_single_oracles(c, gpi, hub)
                out.append((f"{c.id} {tag}update {'gpi' if gpi else 'own'}", g64, r32, info))
        steps, _ = psi_all_oracles(c, hub, steps=1 if hub else 2)
        for j, step in enumerate(steps):
            for i, (g64, r32, info) in enumerate(step):
                out.append((f"{c.id} {tag}all-task step {j + 1} head {i}", dict(psi=g64), dict(psi=r32), info))
    return out


def tsf_records(K: int, B: int, gpi: bool):
    seed = TSF_SEEDS.get((K, B), 0)
    out = [(f"tsf K{K} B{B} {'gpi' if gpi else 'own'} update {j + 1}", g64, r32, info)
           for j, (g64, r32, info) in enumerate(tsf_oracles(K, B, gpi, seed))]
    return out


def tsf_test_records(K: int):
    return [(f"tsf test K{K} step {j + 1}", g64, r32, None)
            for j, (g64, r32) in enumerate(tsf_test_oracles(K, TSF_SEEDS.get((K, 7), 0)))]


def phi_records(c: PhiCase, gpi: bool, transform: bool):
    g64, r32, info = phi_oracles(c, gpi, transform, PHI_SEEDS.get(c.id, 0))
    return [(f"{'tsf-phi' if transform else 'phi'} {c.id} {'gpi' if gpi else 'own'}", g64, r32, info)]


def phi_test_records(hid: int, d: int):
    (t64, t32), (s64, s32) = phi_test_oracles(hid, d, PHI_TEST_SEEDS.get((hid, d), 0))
    return [(f"tsf-phi test hid{hid} d{d}", t64, t32, None), (f"phi test hid{hid} d{d}", s64, s32, None)]


def check_clamp_case(info: Info):
    """The ×40 rewards case: the clamp bites in the φ net, w, its bias, g_i and h, and not in ψ."""
    for k in ("phi", "w", "wb", "g", "h"):
        assert info.clamped[k] > 0, f"the clamp does not reach {k}: {info.clamped}"
    assert info.clamped["psi"] == 0 and info.psi_max < 1, info


def _first_seed(store, key, records, extra=lambda info: None, tries=200):
    for seed in range(tries):
        store[key] = seed
        try:
            for label, _, _, info in records():
                if info is not None:
                    info.check(label)
                    extra(info)
            return seed
        except AssertionError:
            continue
    raise SystemExit(f"no seed for {key}")


if __name__ == "__main__":   # the seeds of the cases: the first for which the input conditions hold
    import dataclasses
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "deep-successor-features-for-transfer_amd"))
    for c in PSI_CASES:
        box = {}
        cc = [c]

        def recs():
            cc[0] = dataclasses.replace(c, seed=box["s"])
            return psi_records(cc[0])

        print("psi", c.id, _first_seed(box, "s", recs), flush=True)
    for K, B in sorted({(K, B) for K, B, _ in TSF_CASES}):
        _first_seed(TSF_SEEDS, (K, B), lambda: tsf_records(K, B, True) + tsf_records(K, B, False))
    print("TSF_SEEDS =", TSF_SEEDS, flush=True)

    def no_clamp(info):
        assert info.psi_max < 1 and not any(info.clamped.values()), info

    for c in PHI_CASES + [CLAMP_CASE]:
        _first_seed(PHI_SEEDS, c.id, lambda: [r for gpi in (True, False) for tr in (True, False)
                                              for r in phi_records(c, gpi, tr)
                                              if c is not CLAMP_CASE or (tr and gpi)],
                    check_clamp_case if c is CLAMP_CASE else no_clamp)
    print("PHI_SEEDS =", PHI_SEEDS, flush=True)
