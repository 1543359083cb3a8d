"""Pre-training of the reward features φ: PreEngine (the sfx_pre_* handle), pre_train (the reference's loop)
and LearntPhi (what the loop leaves as the agent's feature function).

The single-file learned-φ agents open every run with pre_train(train_tasks, 5_000) (sfdqn_phi.py:800-873, :987;
tsfdqn_phi.py:1036-1109, :1230): n_cycles × T × n random-policy env steps, each followed by one minibatch update of
a PhiFunction net (sfdqn_phi.py:90-123) and of the task's reward row.  Here the update is one library call with no
host read; the losses stay on the device until the loop ends.
"""
from __future__ import annotations

import ctypes as C
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check, fptr, lib, stream_ptr

ADAM_DEFAULTS = dict(lr_phi=1e-3, wd_phi=0.0, lr_w=1e-3, wd_w=0.0, betas=(0.9, 0.999), eps=1e-8)


def layer_dims(n_s: int, d: int, hidden: Sequence[int]) -> List[Tuple[int, int]]:
    """(out, in) of every Linear of the φ net."""
    widths = [2 * n_s + 1] + [int(h) for h in hidden] + [d]
    return [(widths[i + 1], widths[i]) for i in range(len(widths) - 1)]


def phi_numel(n_s: int, d: int, hidden: Sequence[int]) -> int:
    return sum(o * (i + 1) for o, i in layer_dims(n_s, d, hidden))


class PhiModule(torch.nn.Module):
    """A torch module with PhiFunction's parameter names (_model.{0,2,4,...}.{weight,bias}) and call forms."""

    def __init__(self, n_s: int, d: int, hidden: Sequence[int] = (128, 256)):
        super().__init__()
        layers = []
        for j, (o, i) in enumerate(layer_dims(n_s, d, hidden)):
            layers += [torch.nn.ReLU()] if j else []
            layers.append(torch.nn.Linear(i, o))
        self._model = torch.nn.Sequential(*layers)

    def forward(self, state, action, next_state):
        state, action, next_state = _call_forms(state, action, next_state)
        return self._model(torch.cat([state, action.to(state.dtype), next_state], dim=1))


def _call_forms(state, action, next_state):
    """PhiFunction.forward's argument forms (sfdqn_phi.py:109-118): a 0-d or 1-d action, 1-d states."""
    action = torch.as_tensor(action)
    if action.ndim == 0:
        action = action.unsqueeze(0)
    if action.ndim == 1:
        action = action.unsqueeze(1)
    state, next_state = torch.as_tensor(state), torch.as_tensor(next_state)
    if state.ndim == 1:
        state = state.unsqueeze(0)
    if next_state.ndim == 1:
        next_state = next_state.unsqueeze(0)
    return state, action, next_state


def pack_module(module: torch.nn.Module) -> torch.Tensor:
    """torch parameters() packing: W [out][in] then b [out] per Linear."""
    return torch.cat([p.detach().reshape(-1).float().cpu() for p in module.parameters()])


class PreEngine:
    """The φ net, its Adam, and T reward rows with theirs, on one GPU (include/sfx.h sfx_pre_*)."""

    ROWS_MAX = 65536     # sfx_pre_features_rows' limit on the rows of one launch

    def __init__(self, n_s: int, d: int, T: int, hidden: Sequence[int] = (128, 256), max_batch: int = 32,
                 device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("PreEngine needs a HIP device (libsfx.so has no CPU path)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_s, self.d, self.T, self.hidden, self.max_batch = n_s, d, T, tuple(int(h) for h in hidden), max_batch
        hid = (C.c_int * max(1, len(self.hidden)))(*self.hidden)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.sfx_pre_create(C.byref(h), n_s, d, T, hid, len(self.hidden), max_batch), "sfx_pre_create")
        self._h = h
        self.P = lib.sfx_pre_numel(h)
        self.adam_hp = dict(ADAM_DEFAULTS)

    def close(self):
        if getattr(self, "_h", None):
            lib.sfx_pre_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ---------------------------------------------------------------- state
    def set_adam(self, lr_phi=1e-3, wd_phi=0.0, lr_w=1e-3, wd_w=0.0, betas=(0.9, 0.999), eps=1e-8):
        check(lib.sfx_pre_set_adam(self._h, lr_phi, wd_phi, lr_w, wd_w, betas[0], betas[1], eps), "sfx_pre_set_adam")
        self.adam_hp = dict(lr_phi=lr_phi, wd_phi=wd_phi, lr_w=lr_w, wd_w=wd_w, betas=tuple(betas), eps=eps)

    @staticmethod
    def _host(x, n) -> np.ndarray:
        a = np.ascontiguousarray(torch.as_tensor(x).detach().cpu().reshape(-1).numpy(), dtype=np.float32)
        if a.size != n:
            raise ValueError(f"expected {n} floats, got {a.size}")
        return a

    def load(self, flat):
        check(lib.sfx_pre_load(self._h, fptr(self._host(flat, self.P))), "sfx_pre_load")

    def get(self) -> torch.Tensor:
        out = np.empty(self.P, np.float32)
        check(lib.sfx_pre_get(self._h, fptr(out)), "sfx_pre_get")
        return torch.from_numpy(out)

    def load_adam(self, m, v, step: int):
        check(lib.sfx_pre_load_adam(self._h, fptr(self._host(m, self.P)), fptr(self._host(v, self.P)), int(step)),
              "sfx_pre_load_adam")

    def get_adam(self) -> Tuple[torch.Tensor, torch.Tensor, int]:
        m, v, step = np.empty(self.P, np.float32), np.empty(self.P, np.float32), C.c_int()
        check(lib.sfx_pre_get_adam(self._h, fptr(m), fptr(v), C.byref(step)), "sfx_pre_get_adam")
        return torch.from_numpy(m), torch.from_numpy(v), step.value

    def load_w(self, t: int, w, m=None, v=None, step: int = 0):
        z = np.zeros(self.d, np.float32)
        check(lib.sfx_pre_load_w(self._h, int(t), fptr(self._host(w, self.d)),
                                 fptr(z if m is None else self._host(m, self.d)),
                                 fptr(z if v is None else self._host(v, self.d)), int(step)), "sfx_pre_load_w")

    def get_w(self, t: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
        w, m, v = (np.empty(self.d, np.float32) for _ in range(3))
        step = C.c_int()
        check(lib.sfx_pre_get_w(self._h, int(t), fptr(w), fptr(m), fptr(v), C.byref(step)), "sfx_pre_get_w")
        return torch.from_numpy(w), torch.from_numpy(m), torch.from_numpy(v), step.value

    # ---------------------------------------------------------------- compute
    def _dev(self, x, dtype) -> torch.Tensor:
        return torch.as_tensor(x).to(device=self.device, dtype=dtype).contiguous()

    def _bind_stream(self):
        check(lib.sfx_pre_set_stream(self._h, C.c_void_p(stream_ptr(self.device.index))), "sfx_pre_set_stream")

    def update(self, task: int, S, a, r, S1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One minibatch update of task `task`; the loss as a device tensor of one element (`out` if given)."""
        S, S1 = self._dev(S, torch.float32).reshape(-1, self.n_s), self._dev(S1, torch.float32).reshape(-1, self.n_s)
        a, r = self._dev(a, torch.long).reshape(-1), self._dev(r, torch.float32).reshape(-1)
        B = S.shape[0]
        if not (S1.shape[0] == a.numel() == r.numel() == B):
            raise ValueError("S, a, r, S1 disagree on the number of rows")
        if out is None:
            out = torch.empty(1, dtype=torch.float32, device=self.device)
        elif not (out.dtype == torch.float32 and out.device == self.device and out.numel() == 1):
            raise ValueError("out: one float32 element on the engine's device")
        self._bind_stream()
        check(lib.sfx_pre_update(self._h, int(task), S.data_ptr(), a.data_ptr(), r.data_ptr(), S1.data_ptr(), B,
                                 out.data_ptr()), "sfx_pre_update")
        return out

    def features(self, S, a, S1) -> torch.Tensor:
        """φ [B, d] of the current net: one sfx_pre_features_rows launch whatever max_batch is (up to ROWS_MAX rows
        a launch); row b equals the one-row call bit for bit."""
        S, S1 = self._dev(S, torch.float32).reshape(-1, self.n_s), self._dev(S1, torch.float32).reshape(-1, self.n_s)
        a = self._dev(a, torch.long).reshape(-1)
        B = S.shape[0]
        if not (S1.shape[0] == a.numel() == B):
            raise ValueError("S, a, S1 disagree on the number of rows")
        out = torch.empty(B, self.d, dtype=torch.float32, device=self.device)
        self._bind_stream()
        for lo in range(0, B, self.ROWS_MAX):
            n = min(self.ROWS_MAX, B - lo)
            check(lib.sfx_pre_features_rows(self._h, S[lo:].data_ptr(), a[lo:].data_ptr(), S1[lo:].data_ptr(), n,
                                            out[lo:].data_ptr()), "sfx_pre_features_rows")
        return out


class LearntPhi:
    """The frozen feature function (`self.learnt_phi` of the single-file agents), callable as PhiFunction.forward
    is (sfdqn_phi.py:109-120): a 0-d or 1-d action, int64 (sfdqn_phi.py) or float32 (tsfdqn_phi.py:1077), and 1-d
    or 2-d states.  Returns a tensor [B, d] on the engine's device."""

    def __init__(self, engine):
        self.engine = engine

    def __call__(self, state, action, next_state) -> torch.Tensor:
        state, action, next_state = _call_forms(state, action, next_state)
        if action.is_floating_point():
            action = action.round()
        return self.engine.features(state, action.reshape(-1).to(torch.long), next_state)

    forward = __call__

    def set_eval(self):
        """PhiFunction.set_eval: no dropout or batch norm in this net, nothing to switch."""

    def to_module(self) -> PhiModule:
        e = self.engine
        mod = PhiModule(e.n_s, e.d, e.hidden)
        flat, off = e.get(), 0
        with torch.no_grad():
            for p in mod.parameters():
                p.copy_(flat[off:off + p.numel()].view_as(p))
                off += p.numel()
        return mod.eval()


def _row(x, n) -> np.ndarray:
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float32).reshape(n)


class _Stage:
    """The minibatch of one step: gathered from the host ring into one buffer (a | S | S1 | r), one copy to the
    device.  With a GPU engine the buffer is a ring of pinned slots, each reused once its copy has completed."""
    SLOTS = 4

    def __init__(self, n_s: int, B: int, device: torch.device):
        self.n_s, self.B, self.device = n_s, B, device
        self.nbytes = (8 * B + 4 * B * (2 * n_s + 1) + 15) // 16 * 16     # slots stay aligned for the int64 view
        cuda = device.type == "cuda"
        self.host = torch.empty(self.SLOTS if cuda else 1, self.nbytes, dtype=torch.uint8, pin_memory=cuda)
        self.np = self.host.numpy()
        self.ev = [None] * self.host.shape[0]
        self.dev = torch.empty(self.nbytes, dtype=torch.uint8, device=device) if cuda else None
        self.i = 0

    def views(self, buf):
        B, n_s = self.B, self.n_s
        o1, o2, o3 = 8 * B, 8 * B + 4 * B * n_s, 8 * B + 8 * B * n_s
        return (buf[:o1].view(torch.long), buf[o1:o2].view(torch.float32).view(B, n_s),
                buf[o2:o3].view(torch.float32).view(B, n_s), buf[o3:o3 + 4 * B].view(torch.float32))

    def put(self, S, a, r, S1, idx):
        i = self.i
        self.i = (i + 1) % self.host.shape[0]
        if self.ev[i] is not None:
            self.ev[i].synchronize()
        ha, hs, hs1, hr = self.views(self.host[i])
        np.take(a, idx, out=ha.numpy())
        np.take(S, idx, axis=0, out=hs.numpy())
        np.take(S1, idx, axis=0, out=hs1.numpy())
        np.take(r, idx, out=hr.numpy())
        if self.dev is None:
            return ha, hs, hs1, hr
        self.dev.copy_(self.host[i], non_blocking=True)
        ev = self.ev[i] = self.ev[i] or torch.cuda.Event()
        ev.record()
        return self.views(self.dev)


def pre_train(train_tasks, n_samples_pre_train: int, n_cycles: int = 5, *, hidden: Sequence[int] = (128, 256),
              engine=None, n_batch: int = 32, n_buffer: int = 1000000, device=None):
    """SFDQN.pre_train (sfdqn_phi.py:800-873; TSFDQN.pre_train, tsfdqn_phi.py:1036-1109) -> (LearntPhi, losses).

    The RNGs are consumed in the reference's order: torch's by PhiFunction's init (the module is built on the CPU
    and packed), then per task by the Linear(d, 1) init and the uniform_(-0.01, 0.01) that replaces it; `random` by
    randrange(n_actions) per step; np.random by randint per replay, once the buffer holds n_batch transitions.
    The buffer is a host ring (the reference's ReplayBuffer: 1 000 000 slots, batches of 32); the losses stay on
    the device and are read back once.

    engine: None builds a PreEngine on `device`; otherwise any object with load(flat), load_w(t, w), `device`,
    update(task, S, a, r, S1, out=) and features(S, a, S1) -- tests drive the loop with a torch restatement."""
    first = train_tasks[0]
    n_actions, n_s, d, T = first.action_count(), int(first.encode_dim()), int(first.feature_dim()), len(train_tasks)
    if int(first.action_dim()) != 1:
        raise ValueError("the φ net takes the action as one input column (action_dim() == 1)")
    module = PhiModule(n_s, d, hidden)     # the draws of PhiFunction.__init__'s Linears, in its order
    if engine is None:
        engine = PreEngine(n_s, d, T, hidden, max_batch=n_batch, device=device)
    engine.load(pack_module(module))
    for t, task in enumerate(train_tasks):
        fit_w = torch.nn.Linear(task.feature_dim(), 1, bias=False)     # its init draw, as the reference makes it
        del fit_w
        engine.load_w(t, torch.Tensor(1, task.feature_dim()).uniform_(-0.01, 0.01).reshape(-1))
    dev = torch.device(engine.device)
    total = n_cycles * T * n_samples_pre_train
    cap = min(int(n_buffer), max(total, 1))
    S, S1 = np.empty((cap, n_s), np.float32), np.empty((cap, n_s), np.float32)
    A, R = np.empty(cap, np.int64), np.empty(cap, np.float32)
    size = index = n_upd = 0
    losses = torch.zeros(max(total, 1), dtype=torch.float32, device=dev)
    stage = _Stage(n_s, n_batch, dev)
    for _cycle in range(n_cycles):
        for t, task in enumerate(train_tasks):
            s_enc = _row(task.encode(task.initialize()), n_s)
            for _sample in range(n_samples_pre_train):
                a = random.randrange(n_actions)
                s1, r, terminal = task.transition(a)
                s1_enc = _row(task.encode(s1), n_s)
                S[index], A[index], R[index], S1[index] = s_enc, a, np.float32(r), s1_enc
                size, index = min(size + 1, cap), (index + 1) % cap
                s_enc = s1_enc
                if terminal:
                    s_enc = _row(task.encode(task.initialize()), n_s)
                if size < n_batch:
                    continue
                idx = np.random.randint(low=0, high=size, size=(n_batch,))
                da, ds, ds1, dr = stage.put(S, A, R, S1, idx)
                engine.update(t, ds, da, dr, ds1, out=losses[n_upd:n_upd + 1])
                n_upd += 1
    return LearntPhi(engine), losses[:n_upd].cpu().tolist()
