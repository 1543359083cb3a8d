"""The φ pre-training update in torch: sfdqn_phi.py:90-123 (PhiFunction) and :800-873 (SFDQN.pre_train).

Generic in dtype: float64 gives the exact answer, float32 on the CPU is the reference's arithmetic (autograd of
mse_loss(r, fit_w(φ(s, a, s1))), then torch's single-tensor Adam, oracle.ref_cpu.adam_, on the φ net with its own
moments and step count and on the task's row with that row's).  RefEngine has the interface of sfx.pretrain.PreEngine,
so sfx.pretrain.pre_train runs over it unchanged; MUTANTS are the wrong updates the float64 budget has to catch.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from sfx.pretrain import ADAM_DEFAULTS, layer_dims, phi_numel

MUTANTS = ("w_with_net_step", "net_step_per_task", "stale_dw0")


def mlp(flat, dims, X, pre: Optional[list] = None):
    y, off = X, 0
    for j, (o, i) in enumerate(dims):
        y = F.linear(y, flat[off:off + o * i].view(o, i), flat[off + o * i:off + o * i + o])
        off += o * i + o
        if j < len(dims) - 1:
            if pre is not None:
                pre.append(y.detach())
            y = torch.relu(y)
    return y


def inputs(S, a, S1, dtype):
    S, S1 = torch.as_tensor(S).to(dtype), torch.as_tensor(S1).to(dtype)
    return torch.cat([S, torch.as_tensor(a).reshape(-1, 1).to(dtype), S1], dim=1)


class RefEngine:
    """The state of one pre-training run (φ net flat in torch packing, rows w [T][d], every moment and step count)
    and its update.  mutant: one of MUTANTS or None."""

    def __init__(self, n_s: int, d: int, T: int, hidden: Sequence[int] = (128, 256), dtype=torch.float32,
                 device="cpu", mutant: Optional[str] = None):
        assert mutant is None or mutant in MUTANTS
        self.n_s, self.d, self.T, self.hidden = n_s, d, T, tuple(hidden)
        self.dims = layer_dims(n_s, d, hidden)
        self.P, self.dtype, self.device, self.mutant = phi_numel(n_s, d, hidden), dtype, torch.device(device), mutant
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=self.device)
        self.flat, self.m, self.v, self.step = z(self.P), z(self.P), z(self.P), 0
        self.w, self.wm, self.wv, self.wstep = z(T, d), z(T, d), z(T, d), [0] * T
        self.adam_hp = dict(ADAM_DEFAULTS)
        self.task_steps = [0] * T          # the net_step_per_task mutant's counters

    def _t(self, x):
        return torch.as_tensor(x).detach().to(device=self.device, dtype=self.dtype).clone()

    # -- the PreEngine interface
    def set_adam(self, lr_phi=1e-3, wd_phi=0.0, lr_w=1e-3, wd_w=0.0, betas=(0.9, 0.999), eps=1e-8):
        self.adam_hp = dict(lr_phi=lr_phi, wd_phi=wd_phi, lr_w=lr_w, wd_w=wd_w, betas=tuple(betas), eps=eps)

    def load(self, flat):
        self.flat = self._t(flat).reshape(-1)
        assert self.flat.numel() == self.P

    def get(self):
        return self.flat.detach().cpu().clone()

    def load_adam(self, m, v, step: int):
        self.m, self.v, self.step = self._t(m).reshape(-1), self._t(v).reshape(-1), int(step)

    def get_adam(self):
        return self.m.cpu().clone(), self.v.cpu().clone(), self.step

    def load_w(self, t, w, m=None, v=None, step: int = 0):
        self.w[t] = self._t(w).reshape(-1)
        self.wm[t] = 0 if m is None else self._t(m).reshape(-1)
        self.wv[t] = 0 if v is None else self._t(v).reshape(-1)
        self.wstep[t] = int(step)

    def get_w(self, t):
        return self.w[t].cpu().clone(), self.wm[t].cpu().clone(), self.wv[t].cpu().clone(), self.wstep[t]

    def features(self, S, a, S1):
        with torch.no_grad():
            return mlp(self.flat, self.dims, inputs(S, a, S1, self.dtype).to(self.device))

    def grads(self, task: int, S, a, r, S1, flat=None, relu_min: bool = False):
        """(loss, dflat, dw_task, smallest |ReLU pre-activation| if asked for, else inf) by autograd."""
        flat = (self.flat if flat is None else flat).detach().clone().requires_grad_(True)
        w = self.w[task].detach().clone().requires_grad_(True)
        pre: List[torch.Tensor] = []
        phi = mlp(flat, self.dims, inputs(S, a, S1, self.dtype).to(self.device), pre)
        r = torch.as_tensor(r).to(device=self.device, dtype=self.dtype).reshape(-1, 1)
        loss = F.mse_loss(r, F.linear(phi, w.view(1, -1)))
        loss.backward()
        return loss.detach(), flat.grad, w.grad, min(float(z.abs().min()) for z in pre) if relu_min else math.inf

    def update(self, task: int, S, a, r, S1, out=None):
        hp = self.adam_hp
        loss, gf, gw, _ = self.grads(task, S, a, r, S1)
        self.step += 1
        self.wstep[task] += 1
        self.task_steps[task] += 1
        k_net = self.task_steps[task] if self.mutant == "net_step_per_task" else self.step
        k_w = self.step if self.mutant == "w_with_net_step" else self.wstep[task]
        kw = dict(betas=hp["betas"], eps=hp["eps"])
        with torch.no_grad():
            if self.mutant == "stale_dw0":
                # the hazard of the launch shape: the upper layers step first, then layer 0's gradient is taken
                # from the stepped weights
                n0 = self.dims[0][0] * (self.dims[0][1] + 1)
                R.adam_(self.flat[n0:], gf[n0:], self.m[n0:], self.v[n0:], k_net, hp["lr_phi"],
                        weight_decay=hp["wd_phi"], **kw)
                mixed = torch.cat([self.flat[:n0], self.flat[n0:]])
                with torch.enable_grad():
                    g0 = self.grads(task, S, a, r, S1, flat=mixed)[1][:n0]
                R.adam_(self.flat[:n0], g0, self.m[:n0], self.v[:n0], k_net, hp["lr_phi"], weight_decay=hp["wd_phi"],
                        **kw)
            else:
                R.adam_(self.flat, gf, self.m, self.v, k_net, hp["lr_phi"], weight_decay=hp["wd_phi"], **kw)
            R.adam_(self.w[task], gw, self.wm[task], self.wv[task], k_w, hp["lr_w"], weight_decay=hp["wd_w"], **kw)
        if out is not None:
            out.copy_(loss.to(out.dtype).reshape(out.shape))
            return out
        return loss.reshape(1)

    # -- for the tests
    def clone(self, dtype=None, mutant=None) -> "RefEngine":
        e = RefEngine(self.n_s, self.d, self.T, self.hidden, dtype or self.dtype, self.device, mutant)
        e.adam_hp = dict(self.adam_hp)
        e.load(self.flat)
        e.load_adam(self.m, self.v, self.step)
        for t in range(self.T):
            e.load_w(t, self.w[t], self.wm[t], self.wv[t], self.wstep[t])
        e.task_steps = list(self.task_steps)
        return e

    def groups(self) -> Dict[str, torch.Tensor]:
        """The parameter groups the budgets are taken over: each W_l, each b_l and the rows w."""
        out, off = {}, 0
        for l, (o, i) in enumerate(self.dims):
            out[f"W{l}"] = self.flat[off:off + o * i]
            out[f"b{l}"] = self.flat[off + o * i:off + o * i + o]
            off += o * i + o
        out["w"] = self.w.reshape(-1)
        return out


def split_groups(dims, flat, w) -> Dict[str, torch.Tensor]:
    """groups() of a packed net and rows that are not in a RefEngine (what a PreEngine returns)."""
    out, off = {}, 0
    flat = torch.as_tensor(flat).reshape(-1)
    for l, (o, i) in enumerate(dims):
        out[f"W{l}"] = flat[off:off + o * i]
        out[f"b{l}"] = flat[off + o * i:off + o * i + o]
        off += o * i + o
    out["w"] = torch.as_tensor(w).reshape(-1)
    return out


def problem(n_s: int, d: int, T: int, hidden: Sequence[int], seed: int, dtype=torch.float32) -> RefEngine:
    """A RefEngine initialised as pre_train initialises (torch's Linear init, rows ~ U(-0.01, 0.01))."""
    gen = torch.Generator().manual_seed(seed)
    e = RefEngine(n_s, d, T, hidden, dtype)
    parts = []
    for o, i in e.dims:
        bound = 1.0 / math.sqrt(i)
        parts += [(torch.rand(o * i, generator=gen) * 2 - 1) * bound, (torch.rand(o, generator=gen) * 2 - 1) * bound]
    e.load(torch.cat(parts))
    for t in range(T):
        e.load_w(t, (torch.rand(d, generator=gen) * 2 - 1) * 0.01)
    return e


def batch(n_s: int, A: int, B: int, gen) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(S, a, r, S1): states ~ N(0, 1), actions uniform, rewards ~ U(0, 1)."""
    S, S1 = torch.randn(B, n_s, generator=gen), torch.randn(B, n_s, generator=gen)
    return S, torch.randint(0, A, (B,), generator=gen), torch.rand(B, generator=gen), S1


def cycle_order(T: int, n_updates: int, per_task: int) -> List[int]:
    """The task of every update when the reference's loop (cycles over tasks, per_task updates each) runs."""
    return [(j // per_task) % T for j in range(n_updates)]


# ---------------------------------------------------------------------------------------------------------------
# the float64 budget of a trajectory
# ---------------------------------------------------------------------------------------------------------------
LOSS_RTOL = 1e-5     # as test_phi_error_budget_vs_float64
FACTOR = 2.0         # another summation order than the float32 restatement's, as in the project's other budgets
ROWS: List[Tuple[str, float, float, float]] = []


def budget_check(what: str, got: Dict[str, torch.Tensor], got_losses, e32: RefEngine, losses32, e64: RefEngine,
                 losses64) -> None:
    """Per group: max |got - p64| <= FACTOR · max |p32 - p64| + one fp32 ulp of the group's largest magnitude;
    every loss within LOSS_RTOL of float64's.  Appends one row per group to ROWS and asserts."""
    g32, g64 = e32.groups(), e64.groups()
    bad = []
    for name, p64 in g64.items():
        p64 = p64.detach().cpu().double()
        err = float((torch.as_tensor(got[name]).detach().cpu().double() - p64).abs().max())
        ref = float((g32[name].detach().cpu().double() - p64).abs().max())
        ulp = float(torch.finfo(torch.float32).eps * p64.abs().max())
        ROWS.append((f"{what} {name}", err, ref, FACTOR * ref + ulp))
        print(f"| {what} {name} | {err:.3e} | {ref:.3e} | {FACTOR * ref + ulp:.3e} |")
        if not err <= FACTOR * ref + ulp:
            bad.append((name, err, ref))
    lg, l64 = torch.as_tensor(got_losses).double().reshape(-1), torch.as_tensor(losses64).double().reshape(-1)
    assert lg.numel() == l64.numel()
    rel = float(((lg - l64).abs() / l64.abs().clamp_min(1e-30)).max())
    print(f"| {what} losses | {rel:.3e} | {float(((torch.as_tensor(losses32).double().reshape(-1) - l64).abs() / l64.abs().clamp_min(1e-30)).max()):.3e} | {LOSS_RTOL:.0e} |")
    assert not bad, f"{what}: groups out of the float64 budget: {bad}"
    assert rel <= LOSS_RTOL, f"{what}: a loss {rel:.3e} (relative) from float64's"


def run(e: RefEngine, batches, order) -> List[float]:
    return [float(e.update(t, *b)) for t, b in zip(order, batches)]


# ---------------------------------------------------------------------------------------------------------------
# the synthetic tasks of tests/golden/pretrain_phi.npz (tools/gen_pretrain_golden.py)
# ---------------------------------------------------------------------------------------------------------------
class SynthTask:
    """The part of tasks/task.py's interface that pre_train uses.  All its randomness comes from a generator of its
    own, so the global `random` / np.random / torch states after a run record the loop's draws and nothing else."""

    def __init__(self, n_s: int, A: int, d: int, idx: int, episode: int = 7):
        import numpy as np

        self.n_s, self.A, self.d, self.idx, self.episode = n_s, A, d, idx, episode
        self.rng = np.random.RandomState(9100 + idx)
        self.M = (self.rng.randn(A, n_s, n_s) * 0.5).astype(np.float32)
        self.c = self.rng.randn(n_s).astype(np.float32)
        self.s, self.k = None, 0

    def action_count(self):
        return self.A

    def action_dim(self):
        return 1

    def encode_dim(self):
        return self.n_s

    def feature_dim(self):
        return self.d

    def initialize(self):
        import numpy as np

        self.s, self.k = self.rng.randn(self.n_s).astype(np.float32), 0
        return self.s

    def transition(self, a: int):
        import numpy as np

        s1 = np.tanh(self.M[a] @ self.s + 0.3 * self.rng.randn(self.n_s).astype(np.float32)).astype(np.float32)
        r = float(self.c @ s1) + 0.1 * a
        self.s, self.k = s1, self.k + 1
        return s1, r, self.k % self.episode == 0

    def encode(self, s):
        return torch.tensor(s, dtype=torch.float32).reshape(1, -1)


def seed_all(seed: int) -> None:
    import random

    import numpy as np

    random.seed(seed)
    np.random.seed(seed + 1)
    torch.manual_seed(seed + 2)


def rng_states() -> Dict[str, "object"]:
    """The global generators' states as arrays (what the fixture records and the tests compare)."""
    import random

    import numpy as np

    rs, ns = random.getstate(), np.random.get_state()
    return dict(rng_random=np.array(rs[1], dtype=np.int64), rng_numpy=np.array(ns[1], dtype=np.int64),
                rng_numpy_pos=np.int64(ns[2]), rng_torch=torch.get_rng_state().numpy().copy())
